"""Force matching for three hidden layers (htf.DescriptorMLP(trainable="deep", H3=...), deep_loss_gradient) on the host: the
layer's new value of ``trainable``, the C ABI table of include/htf_cfw3train.h and the argument checks of its two entry points.
No GPU."""
import ctypes

import pytest
import torch

KW = dict(K=8, H1=12, H2=10, device="cpu")


def test_deep_layer_value(htf):
    lay = htf.DescriptorMLP(H3=7, trainable="deep", **KW)
    assert lay.trainable == "deep" and lay.dense == "mfma" and lay.conservative is True and lay.H3 == 7
    cfg = lay.get_config()
    assert (cfg["trainable"], cfg["dense"], cfg["conservative"], cfg["H3"]) == ("deep", "mfma", True, 7)
    again = htf.DescriptorMLP(device="cpu", **cfg)
    assert again.trainable == "deep" and again.get_config() == cfg
    with pytest.raises(ValueError, match=r"H3.*trainable=\"wide\""):
        htf.DescriptorMLP(trainable="deep", **KW)
    for bad, word in ((dict(l_max=1), "l_max"), (dict(n_models=2), "n_models"), (dict(dense="split16"), "split16")):
        with pytest.raises(NotImplementedError, match=r"H3.*%s.*two-hidden-layer" % word):
            htf.DescriptorMLP(H3=7, trainable="deep", **dict(KW, **bad))
    with pytest.raises(ValueError, match="trainable must be.*'wide' or 'deep'"):
        htf.DescriptorMLP(trainable="narrow", **KW)


def test_deep_method_checks(htf):
    """Callable on any H3 layer, with no CPU path; the others are pointed to their own sweep."""
    x, labels, idx = torch.zeros((4, 16, 4)), torch.zeros((4, 4)), torch.zeros((4, 16), dtype=torch.int32)
    for kw in (dict(trainable="deep"), dict(conservative=True, dense="mfma")):
        with pytest.raises(ValueError, match="device tensor"):
            htf.DescriptorMLP(H3=7, **dict(KW, **kw)).deep_loss_gradient(x, labels, idx)
    for kw in (dict(), dict(trainable="wide"), dict(trainable="total")):
        with pytest.raises(ValueError, match=r"H3.*wide_loss_gradient.*total_loss_gradient"):
            htf.DescriptorMLP(**dict(KW, **kw)).deep_loss_gradient(x, labels, idx)
    with pytest.raises(NotImplementedError, match="angular_loss_gradient"):
        htf.DescriptorMLP(conservative=True, l_max=1, **KW).deep_loss_gradient(x, labels, idx)
    with pytest.raises(NotImplementedError, match=r"member\(m\)\.deep_loss_gradient"):
        htf.DescriptorMLP(conservative=True, n_models=2, **KW).deep_loss_gradient(x, labels, idx)


def test_cfw3t_abi_table(htf):
    L = htf._lib
    assert sorted(L.CFW3T_PROTOTYPES) == ["htf_cfw3_loss_grad", "htf_cfw3_scratch_floats"]
    every, raw = [n for n, _ in L.ALL_PROTOTYPES], ctypes.CDLL(L.LIB_PATH)
    for n in L.CFW3T_PROTOTYPES:
        assert hasattr(raw, n) and hasattr(L.lib, n) and every.count(n) == 1
    ct = L.CT_PROTOTYPES["htf_ct_loss_grad"][1]
    assert L.CFW3T_PROTOTYPES["htf_cfw3_loss_grad"][1] == ct[:9] + [ctypes.c_uint] + ct[9:]
    assert L.CFW3T_PROTOTYPES["htf_cfw3_scratch_floats"][0] is ctypes.c_size_t


def test_cfw3_loss_grad_argument_errors(htf):
    """Checked ahead of any launch (no device needed): HTF_ERR_INVALID and a message that starts "descriptor network"."""
    L = htf._lib
    mu, w = torch.zeros(8), torch.zeros(8 * 256 + 256 + 2 * (256 * 256 + 256) + 256 + 1)
    args = dict(nlist=0x1000, dt=L.HTF_F32, index=0x6000, B=4, NN=16, K=8, T=1, H1=256, H2=256, H3=256, act=L.ACT_TANH,
                w=w.data_ptr(), mu=mu.data_ptr(), gap=0.5, rho=0x3000, accum=0x4000, scratch=0x5000, rows=None, n_rows=4, rc=0.0)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_cfw3_loss_grad(a["nlist"], a["dt"], a["index"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["H3"],
                                        a["act"], a["w"], a["mu"], a["gap"], a["rho"], a["accum"], a["scratch"], a["rows"],
                                        a["n_rows"], a["rc"], None)

    for bad in (dict(H1=257), dict(H2=0), dict(H3=0), dict(H3=257), dict(K=33, T=2), dict(NN=257), dict(n_rows=5), dict(w=None),
                dict(rho=None), dict(accum=None), dict(scratch=None), dict(index=None), dict(act=7), dict(rc=-1.0), dict(gap=0.0)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert L.last_error().startswith("descriptor network"), L.last_error()
    assert call(B=0, n_rows=0, nlist=None, index=None, rho=None, accum=None, scratch=None) == L.HTF_OK


def test_cfw3_scratch_floats(htf):
    """One partial [1 + P] per block: a block per tile, at most 256; tiles of 32 rows up to 608 image lines, of 16 above; 0 for
    what the sweep refuses."""
    f = htf._lib.lib.htf_cfw3_scratch_floats
    P = 64 * 256 + 256 + 2 * (256 * 256 + 256) + 256 + 1      # 64 + 3 x 256 = 832 lines: 16 rows
    assert f(0, 16, 4, 256, 256, 256) == 0
    for n, blocks in ((1, 1), (16, 1), (17, 2), (343, 22), (4096, 256), (1 << 20, 256)):
        assert f(n, 16, 4, 256, 256, 256) == blocks * (1 + P), n
    Q = 64 * 160 + 160 + 160 * 128 + 128 + 128 * 96 + 96 + 96 + 1   # 448 lines: 32 rows
    for n, blocks in ((32, 1), (33, 2), (343, 11), (8192, 256), (1 << 20, 256)):
        assert f(n, 16, 4, 160, 128, 96) == blocks * (1 + Q), n
    # the switch, at 64 + 256 + 192 + 96 = 608 lines
    for h2, blocks in ((192, 11), (193, 22)):
        assert f(343, 16, 4, 256, h2, 96) == blocks * (1 + 64 * 256 + 256 + 256 * h2 + h2 + h2 * 96 + 96 + 96 + 1), h2
    assert f(4, 1, 1, 8, 8, 8) == 0 and f(4, 8, 1, 257, 8, 8) == 0 and f(4, 8, 1, 8, 8, 0) == 0 and f(4, 33, 2, 8, 8, 8) == 0
