"""htf.DescriptorMLP(dense="mfma", H3=...) on the host: the layer's ``H3`` argument and its eight weight arrays, the initialiser,
the export of include/htf_cfwide3.h's entry and its argument checks.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

KW = dict(K=8, H1=12, H2=10, device="cpu", conservative=True, dense="mfma")


def test_cfw3_layer_arguments(htf):
    lay = htf.DescriptorMLP(K=16, n_types=4, H1=256, H2=240, H3=96, device="cpu", conservative=True, dense="mfma")
    assert lay.H3 == 96 and lay.P == lay.w.numel() == 64 * 256 + 256 + 256 * 240 + 240 + 240 * 96 + 96 + 96 + 1
    for bad in (0, 257, 2.5, True, "8"):
        with pytest.raises(ValueError, match="H3"):
            htf.DescriptorMLP(H3=bad, **KW)
    for bad in (dict(conservative=False), dict(dense="lanes")):
        with pytest.raises(ValueError, match=r"H3.*conservative=True and dense=\"mfma\""):
            htf.DescriptorMLP(H3=8, **dict(KW, **bad))
    for bad, word in ((dict(l_max=1), "l_max"), (dict(n_models=2), "n_models"), (dict(dense="split16"), "split16"),
                      (dict(trainable="wide"), "trainable"), (dict(trainable="total"), "trainable"), (dict(trainable=True), "trainable")):
        with pytest.raises(NotImplementedError, match=r"H3.*%s.*two-hidden-layer" % word):
            htf.DescriptorMLP(H3=8, **dict(KW, **bad))
    x, idx, lab = torch.zeros((4, 16, 4)), torch.zeros((4, 16), dtype=torch.int32), torch.zeros((4, 4))
    for what, call in (("forces", lambda: lay.forces(x)), ("loss_gradient", lambda: lay.loss_gradient(x, lab)),
                       ("total_loss_gradient", lambda: lay.total_loss_gradient(x, lab, idx)),
                       ("wide_loss_gradient", lambda: lay.wide_loss_gradient(x, lab, idx))):
        with pytest.raises(NotImplementedError, match=r"%s\(\).*H3" % what):
            call()


@pytest.mark.parametrize("S", [1, 3])
def test_cfw3_weights(htf, tmp_path, S):
    """Eight arrays in Keras order, flat in ``w``, through get / set / save / load and the species axis."""
    lay = htf.DescriptorMLP(H3=7, n_species=S, **KW)
    lead = (S,) if S > 1 else ()
    shapes = [(8, 12), (12,), (12, 10), (10,), (10, 7), (7,), (7, 1), (1,)]
    ws = lay.get_weights()
    assert [w.shape for w in ws] == [lead + s for s in shapes]
    assert lay.P == sum(int(np.prod(s)) for s in shapes) and lay.w.numel() == S * lay.P
    assert np.array_equal(np.concatenate([w.reshape(S, -1) for w in ws], axis=1).ravel(), lay.w.numpy())
    new = [np.random.default_rng(i).standard_normal(w.shape).astype(np.float32) for i, w in enumerate(ws)]
    lay.set_weights(new)
    assert np.array_equal(lay.w.numpy()[-1:], new[7].ravel()[-1:])   # b4 of the last network is the last float
    lay.save_weights(str(tmp_path / "w.npz"))
    other = htf.DescriptorMLP(H3=7, n_species=S, seed=9, **KW)
    other.load_weights(str(tmp_path / "w.npz"))
    assert torch.equal(other.w, lay.w)
    with pytest.raises(ValueError, match="shape"):
        lay.set_weights(new[:4] + [new[4][..., :6]] + new[5:])
    with pytest.raises(ValueError, match="8 weight arrays"):
        lay.set_weights(new[:6])


def test_cfw3_config_and_initialiser(htf):
    assert "H3" not in htf.DescriptorMLP(**KW).get_config()
    cfg = htf.DescriptorMLP(H3=200, r_cut=2.5, **KW).get_config()
    assert cfg["H3"] == 200 and cfg["dense"] == "mfma"
    again = htf.DescriptorMLP(device="cpu", **cfg)
    assert again.H3 == 200 and again.get_config() == cfg
    from hoomd_tf_amd.initializers import glorot_uniform, mlp_params
    a, b = mlp_params(seed=5, K=8, H1=12, H2=10, bias_scale=0.1), mlp_params(seed=5, K=8, H1=12, H2=10, bias_scale=0.1, H3=None)
    assert list(a) == list(b) == ["W1", "b1", "W2", "b2", "W3", "b3"] and all(np.array_equal(a[k], b[k]) for k in a)
    p, rng = mlp_params(seed=5, K=8, H1=12, H2=10, H3=7), np.random.default_rng(5)
    for k, (m, n) in zip(("W1", "W2", "W3", "W4"), ((8, 12), (12, 10), (10, 7), (7, 1))):
        assert np.array_equal(p[k], glorot_uniform(rng, m, n))
    assert p["b3"].shape == (7,) and p["b4"].shape == (1,)


def test_cfw3_entry_point(htf):
    """Exported, bound, and checked ahead of any launch: HTF_ERR_INVALID and a message (no device needed)."""
    L = htf._lib
    names = [n for n, _ in L.ALL_PROTOTYPES]
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "htf_cfw3_grad") and names.count("htf_cfw3_grad") == 1 and "htf_cfw3_grad" in L.CFW3_PROTOTYPES
    mu, w = torch.zeros(8), torch.zeros(8 * 256 + 256 + 2 * (256 * 256 + 256) + 256 + 1)
    args = dict(nlist=0x1000, dt=L.HTF_F32, B=4, NN=16, K=8, T=1, H1=256, H2=256, H3=256, act=L.ACT_TANH, w=w.data_ptr(),
                mu=mu.data_ptr(), gap=0.5, g=0x2000, e=0x3000, rows=None, n_rows=4, rc=0.0)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_cfw3_grad(a["nlist"], a["dt"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["H3"], a["act"], a["w"],
                                   a["mu"], a["gap"], a["g"], a["e"], a["rows"], a["n_rows"], a["rc"], None)

    for bad in (dict(H1=257), dict(H2=0), dict(H3=0), dict(H3=257), dict(g=None), dict(e=None), dict(K=33, T=2), dict(NN=257),
                dict(n_rows=5), dict(w=None)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert L.last_error().startswith("descriptor network"), L.last_error()
    assert call(n_rows=0) == L.HTF_OK and call(B=0, n_rows=0, nlist=None, g=None, e=None) == L.HTF_OK
