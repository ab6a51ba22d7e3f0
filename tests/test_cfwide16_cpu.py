"""htf.DescriptorMLP(dense="split16") on the host: the layer's ``dense`` argument, the export of include/htf_cfwide16.h's entry
and its argument checks.  No GPU."""
import ctypes

import pytest
import torch


def test_cfw16_layer_arguments(htf):
    lay = htf.DescriptorMLP(K=16, n_types=4, H1=256, H2=256, device="cpu", conservative=True, dense="split16")
    assert lay.dense == "split16" and lay.P == lay.w.numel() == 64 * 256 + 256 + 256 * 256 + 256 + 256 + 1
    assert torch.equal(lay.w, htf.DescriptorMLP(K=16, n_types=4, H1=256, H2=256, device="cpu", conservative=True, dense="mfma").w)
    kw = dict(K=8, H1=8, H2=8, device="cpu")
    for bad, word in ((dict(H1=257, conservative=True), "256"), (dict(), "conservative=True"),
                      (dict(conservative=True, l_max=1), "l_max"), (dict(conservative=True, n_models=2), "n_models"),
                      (dict(trainable="total"), 'trainable="wide"'), (dict(trainable=True), 'trainable="wide"'),
                      (dict(conservative=True, dense="fp16"), "'lanes', 'mfma' or 'split16'")):
        with pytest.raises(ValueError, match=word):
            htf.DescriptorMLP(**dict(dict(kw, dense="split16"), **bad))
    assert htf.DescriptorMLP(trainable="wide", **kw).dense == "mfma"   # "wide" decides the stack itself
    x, idx = torch.zeros((4, 16, 4)), torch.zeros((4, 16), dtype=torch.int32)
    for what, call in (("forces", lambda: lay.forces(x)), ("loss_gradient", lambda: lay.loss_gradient(x, torch.zeros((4, 4)))),
                       ("total_loss_gradient", lambda: lay.total_loss_gradient(x, torch.zeros((4, 4)), idx))):
        with pytest.raises(NotImplementedError, match=r"%s\(\).*split16.*lanes" % what):
            call()


def test_cfw16_config_round_trips(htf):
    cfg = htf.DescriptorMLP(K=8, H1=200, H2=96, device="cpu", conservative=True, dense="split16", r_cut=2.5).get_config()
    assert cfg["dense"] == "split16" and cfg["H1"] == 200
    again = htf.DescriptorMLP(device="cpu", **cfg)
    assert again.dense == "split16" and again.get_config() == cfg


def test_cfw16_entry_point(htf):
    """Exported, bound, and checked ahead of any launch: HTF_ERR_INVALID and a message (no device needed)."""
    L = htf._lib
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "htf_cfw16_grad") and "htf_cfw16_grad" in dict(L.ALL_PROTOTYPES)
    assert list(L.CFW16_PROTOTYPES) == ["htf_cfw16_grad"] and L.CFW16_PROTOTYPES["htf_cfw16_grad"] == L.CFW_PROTOTYPES["htf_cfw_grad"]
    mu, w = torch.zeros(8), torch.zeros(8 * 256 + 256 + 256 * 256 + 256 + 256 + 1)
    args = dict(nlist=0x1000, dt=L.HTF_F32, B=4, NN=16, K=8, T=1, H1=256, H2=256, act=L.ACT_TANH, w=w.data_ptr(), mu=mu.data_ptr(),
                gap=0.5, g=0x2000, e=0x3000, rows=None, n_rows=4, rc=0.0)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_cfw16_grad(a["nlist"], a["dt"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["act"], a["w"], a["mu"],
                                    a["gap"], a["g"], a["e"], a["rows"], a["n_rows"], a["rc"], None)

    for bad in (dict(H1=257), dict(H2=0), dict(g=None), dict(e=None), dict(K=33, T=2), dict(NN=257), dict(n_rows=5), dict(w=None)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    assert call(n_rows=0) == L.HTF_OK and call(B=0, n_rows=0, nlist=None, g=None, e=None) == L.HTF_OK
