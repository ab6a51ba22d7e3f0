"""Force matching for the wide dense stack (htf.DescriptorMLP(trainable="wide"), wide_loss_gradient) on the host: the layer's new
value of ``trainable`` with its refusals, the C ABI table of include/htf_cfwtrain.h and the argument checks of its two entry
points.  No GPU."""
import ctypes

import pytest
import torch


def test_wide_layer_value(htf):
    kw = dict(K=8, device="cpu")
    lay = htf.DescriptorMLP(H1=256, H2=200, trainable="wide", **kw)
    assert lay.trainable == "wide" and lay.dense == "mfma" and lay.conservative is True
    cfg = lay.get_config()
    assert (cfg["trainable"], cfg["dense"], cfg["conservative"], cfg["H1"]) == ("wide", "mfma", True, 256)
    again = htf.DescriptorMLP(device="cpu", **cfg)
    assert again.trainable == "wide" and again.get_config() == cfg
    full = htf.DescriptorMLP(H1=96, H2=80, trainable="wide", r_cut=2.5, n_species=2, n_types=2, **kw).get_config()
    assert htf.DescriptorMLP(device="cpu", **full).get_config() == full
    with pytest.raises(ValueError, match="256"):
        htf.DescriptorMLP(H1=257, H2=8, trainable="wide", **kw)
    with pytest.raises(NotImplementedError, match="l_max"):
        htf.DescriptorMLP(H1=8, H2=8, trainable="wide", l_max=1, **kw)
    with pytest.raises(NotImplementedError, match="n_models"):
        htf.DescriptorMLP(H1=8, H2=8, trainable="wide", n_models=2, **kw)
    with pytest.raises(ValueError, match="trainable must be.*'wide'"):
        htf.DescriptorMLP(H1=8, H2=8, trainable="narrow", **kw)
    # the other values keep refusing the wide stack
    for tr in (True, "total", "angular", "committee"):
        with pytest.raises((ValueError, NotImplementedError)):
            htf.DescriptorMLP(H1=8, H2=8, trainable=tr, dense="mfma", l_max=int(tr == "angular"), n_models=1 + (tr == "committee"), **kw)


def test_wide_method_checks(htf):
    """Callable on any single-network l_max = 0 layer, with no CPU path; the others are pointed to their own sweep."""
    kw = dict(K=8, H1=8, H2=8, device="cpu")
    x, labels, idx = torch.zeros((4, 16, 4)), torch.zeros((4, 4)), torch.zeros((4, 16), dtype=torch.int32)
    for lay in (htf.DescriptorMLP(**kw), htf.DescriptorMLP(trainable="total", **kw), htf.DescriptorMLP(trainable="wide", **kw)):
        with pytest.raises(ValueError, match="device tensor"):
            lay.wide_loss_gradient(x, labels, idx)
    with pytest.raises(NotImplementedError, match="angular_loss_gradient"):
        htf.DescriptorMLP(conservative=True, l_max=1, **kw).wide_loss_gradient(x, labels, idx)
    with pytest.raises(NotImplementedError, match=r"member\(m\)\.wide_loss_gradient"):
        htf.DescriptorMLP(conservative=True, n_models=2, **kw).wide_loss_gradient(x, labels, idx)


def test_cfwt_abi_table(htf):
    L = htf._lib
    assert sorted(L.CFWT_PROTOTYPES) == ["htf_cfw_loss_grad", "htf_cfw_scratch_floats"]
    every = [n for n, _ in L.ALL_PROTOTYPES]
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in L.CFWT_PROTOTYPES:
        assert hasattr(raw, n) and hasattr(L.lib, n) and every.count(n) == 1
    assert L.CFWT_PROTOTYPES["htf_cfw_loss_grad"][1] == L.CT_PROTOTYPES["htf_ct_loss_grad"][1]
    assert L.CFWT_PROTOTYPES["htf_cfw_scratch_floats"][0] is ctypes.c_size_t


def test_cfw_loss_grad_argument_errors(htf):
    """Checked ahead of any launch (no device needed): HTF_ERR_INVALID and a message that starts "descriptor network"."""
    L = htf._lib
    P = 8 * 256 + 256 + 256 * 256 + 256 + 256 + 1
    mu, w = torch.zeros(8), torch.zeros(P)
    args = dict(nlist=0x1000, dt=L.HTF_F32, index=0x6000, B=4, NN=16, K=8, T=1, H1=256, H2=256, act=L.ACT_TANH, w=w.data_ptr(),
                mu=mu.data_ptr(), gap=0.5, rho=0x3000, accum=0x4000, scratch=0x5000, rows=None, n_rows=4, rc=0.0)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_cfw_loss_grad(a["nlist"], a["dt"], a["index"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["act"],
                                       a["w"], a["mu"], a["gap"], a["rho"], a["accum"], a["scratch"], a["rows"], a["n_rows"], a["rc"],
                                       None)

    for bad in (dict(H1=257), dict(H2=0), dict(K=33, T=2), dict(NN=257), dict(n_rows=5), dict(w=None), dict(rho=None),
                dict(accum=None), dict(scratch=None), dict(index=None), dict(act=7), dict(rc=-1.0), dict(gap=0.0)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert L.last_error().startswith("descriptor network"), L.last_error()
    assert call(B=0, n_rows=0, nlist=None, index=None, rho=None, accum=None, scratch=None) == L.HTF_OK


def test_cfw_scratch_floats(htf):
    """One partial [1 + P] per block: a block per tile of 32 rows, at most 256; 0 for what the sweep refuses."""
    f = htf._lib.lib.htf_cfw_scratch_floats
    P = 64 * 256 + 256 + 256 * 256 + 256 + 256 + 1
    assert f(0, 16, 4, 256, 256) == 0
    for n, blocks in ((1, 1), (32, 1), (33, 2), (343, 11), (8192, 256), (1 << 20, 256)):
        assert f(n, 16, 4, 256, 256) == blocks * (1 + P) >= 1 + P, n
    assert f(4, 1, 1, 8, 8) == 0 and f(4, 8, 1, 257, 8) == 0 and f(4, 33, 2, 8, 8) == 0
