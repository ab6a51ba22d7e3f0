"""Force matching on the wide dense stack on the MI355X (csrc/cfwtrain.hip, include/htf_cfwtrain.h;
DescriptorMLP.wide_loss_gradient, trainable="wide") against the reference of test_gpu_desc_total_train.py: torch's fp64 double
backward through the positions, fed the sweep's own fp32 residual.  Systems and layers are test_gpu_desc_total.py's and
test_gpu_desc_wide.py's; every row count is ragged against the tile of 32.

Bound: accum[0] to 1e-5 of the fp64 SSR, and the largest gradient error below 2e-4 sqrt(max(H1, H2, 64) / 64) of the largest
reference entry -- test_gpu_desc_total_train.py's TOL for 64-long fp32 chains with test_gpu_desc_wide.py's square-root growth.

Largest error / largest reference entry measured per case of test_gradient_against_fp64_double_backward, in CASES' order:
9.6e-8, 8.8e-8, 9.6e-8, 1.4e-7, 6.7e-8, 9.5e-8, 7.6e-8, 1.5e-7, 8.2e-7, 3.7e-8; species 8.7e-8 and 4.2e-8; tiled 2.1e-7."""
import math

import pytest
import torch

import test_gpu_desc_total_train as TT
from test_gpu_desc_total import _system
from test_gpu_desc_total_train import _check, _labels, _training_run, reference_gradient
from test_gpu_desc_wide import _wide

pytestmark = pytest.mark.gpu
CAP = 256   # include/htf_cfwtrain.h HTF_CFWT_MAX_BLOCKS: the launcher's grid cap, one block per tile of 32 rows below it


def _bound(monkeypatch, H1, H2):
    """_check asserts against its module's TOL: the chain-length rule of the module docstring for this case."""
    monkeypatch.setattr(TT, "TOL", 2e-4 * math.sqrt(max(H1, H2, 64) / 64.0))


def _case(htf, cuda, config, seed, **kw):
    p, L, rc_list, x, idx = _system(config)
    assert len(p) % 32
    cut = kw.pop("cut", True)
    lay = _wide(htf, high=rc_list, r_cut=0.9 * rc_list if cut else None, seed=seed, **kw)
    return p, L, x, idx, p[:, 3].contiguous(), lay, _labels(len(p), cuda, seed + 2)


# (H1, H2, config, K, n_types, cut, activation, dtype): D = 16, 21 and 64; both activations, cutoffs and dtypes at the top width
CASES = [
    (256, 256, "b256", 16, 4, True, "tanh", torch.float32),
    (256, 256, "a", 16, 1, False, "linear", torch.float64),
    (256, 256, "b", 7, 3, True, "tanh", torch.float64),
    (65, 33, "a", 7, 3, False, "tanh", torch.float32),
    (33, 65, "b256", 16, 1, True, "linear", torch.float64),
    (96, 160, "a", 16, 4, True, "tanh", torch.float32),
    (160, 96, "b", 7, 3, False, "linear", torch.float32),
    (32, 24, "a", 16, 1, True, "tanh", torch.float64),
    (32, 24, "b256", 16, 4, False, "tanh", torch.float32),
    (1, 1, "a", 7, 3, True, "tanh", torch.float32),
]


@pytest.mark.parametrize("H1,H2,config,K,n_types,cut,activation,dtype", CASES)
def test_gradient_against_fp64_double_backward(htf, cuda, monkeypatch, H1, H2, config, K, n_types, cut, activation, dtype):
    p, L, x, idx, types, lay, labels = _case(htf, cuda, config, 5 + n_types, H1=H1, H2=H2, K=K, n_types=n_types, cut=cut,
                                             activation=activation)
    xx = x.to(dtype)
    accum = lay.wide_loss_gradient(xx, labels, idx, types=types)
    assert accum.dtype == torch.float32 and accum.shape == (1 + lay.P,) and torch.isfinite(accum).all()
    pred = lay.total_forces(xx, idx, types=types).to(torch.float32)
    resid = pred - labels
    g = reference_gradient(lay, p, L, x, idx, resid)[0]
    _bound(monkeypatch, H1, H2)
    _check(lay, accum[1:], g, accum[0].item(), (resid.double() ** 2).sum().item(),
           "%d x %d %s D=%d %s cut=%s %s" % (H1, H2, config, K * n_types, activation, cut, dtype))
    assert torch.equal(lay.wide_loss_gradient(xx, labels, idx, pred=pred), accum)   # a prediction handed in is the one evaluated


@pytest.mark.parametrize("config,n_types", [("a", 3), ("b256", 1)])
def test_both_kernels_on_one_layer(htf, cuda, config, n_types):
    p, L, x, idx, types, lay, labels = _case(htf, cuda, config, 9, H1=32, H2=24, n_types=n_types, dense="lanes")
    pred = lay.total_forces(x, idx, types=types).to(torch.float32)
    a, b = lay.wide_loss_gradient(x, labels, idx, pred=pred).double(), lay.total_loss_gradient(x, labels, idx, pred=pred).double()
    err, scale = (a[1:] - b[1:]).abs().max().item(), b[1:].abs().max().item()
    print("%s: max|wide - lanes| = %.3g of %.3g; SSR %.9g vs %.9g" % (config, err, scale, a[0].item(), b[0].item()))
    assert scale > 0 and err < 2e-4 * scale and abs(a[0].item() - b[0].item()) <= 1e-5 * b[0].item()


def test_one_network_per_species(htf, cuda, monkeypatch):
    p, L, x, idx, types, lay, labels = _case(htf, cuda, "a", 11, H1=96, H2=160, K=20, n_types=2, n_species=3)
    sp = (p[:, 3].long() % 2) * 2   # species 1 is absent
    spf = sp.to(torch.float32)
    accum = lay.wide_loss_gradient(x, labels, idx, types=types, species=spf)
    assert accum.shape == (3, 1 + lay.P) and (accum[1] == 0).all()
    resid = lay.total_forces(x, idx, types=types, species=spf).to(torch.float32) - labels
    g = reference_gradient(lay, p, L, x, idx, resid, sp=sp)
    _bound(monkeypatch, 96, 160)
    for s in (0, 2):
        _check(lay, accum[s, 1:], g[s], accum[s, 0].item(), (resid[sp == s].double() ** 2).sum().item(), "species %d" % s)


def test_more_tiles_than_blocks(htf, cuda):
    """Config b's 343 rows 48 times, the index shifted by 343 per copy: 16 464 rows > 2 x 32 x CAP, 515 tiles on CAP blocks, so
    every block adds at least a second tile into its partial.  Reference: 48 x the block's fp64 gradient."""
    rep = 48
    p, L, xb, idxb, types, lay, lb = _case(htf, cuda, "b", 16, H1=32, H2=24)
    nb = len(p)
    x, labels = xb.repeat(rep, 1, 1).contiguous(), lb.repeat(rep, 1).contiguous()
    shift = (nb * torch.arange(rep, dtype=torch.int32, device=cuda)).repeat_interleave(nb)[:, None]
    idx = torch.where(idxb.repeat(rep, 1) >= 0, idxb.repeat(rep, 1) + shift, -1).to(torch.int32).contiguous()
    assert x.shape[0] > 2 * 32 * CAP
    pred_b = lay.total_forces(xb, idxb).to(torch.float32)
    accum = lay.wide_loss_gradient(x, labels, idx, pred=pred_b.repeat(rep, 1).contiguous())
    g = rep * reference_gradient(lay, p, L, xb, idxb, pred_b - lb)[0]
    _check(lay, accum[1:], g, accum[0].item(), rep * ((pred_b - lb).double() ** 2).sum().item(), "tiled x %d" % rep)


def test_bits_and_edges(htf, cuda):
    p, L, x, idx, types, lay, labels = _case(htf, cuda, "b", 14, H1=256, H2=256)
    a = lay.wide_loss_gradient(x, labels, idx)
    assert torch.equal(lay.wide_loss_gradient(x, labels, idx), a) and a[1:].abs().max().item() > 0
    out = torch.full_like(a, float("nan"))
    assert lay.wide_loss_gradient(x, labels, idx, accum=out) is out and torch.equal(out, a)
    for dt in (torch.float32, torch.float64):
        acc = lay.wide_loss_gradient(torch.zeros((0, 32, 4), dtype=dt, device=cuda), torch.zeros((0, 4), dtype=dt, device=cuda),
                                     torch.zeros((0, 32), dtype=torch.int32, device=cuda))
        assert acc.shape == (1 + lay.P,) and (acc == 0).all()


def test_one_sgd_step_through_tfcompute(htf, cuda):
    """After ONE SGD step from fresh weights, w - w0 = -lr g / (4 N), g from wide_loss_gradient on the step's own tensor, index
    and labels; the step is sized from a first, identical run, as test_gpu_desc_total_train.py sizes its own."""
    def layer():
        return htf.DescriptorMLP(K=8, H1=96, H2=80, low=0.5, high=2.5, r_cut=2.0, trainable="wide")

    def run(lr):
        lay = layer()
        w0 = lay.w.clone()
        model, tfc, sysm = _training_run(htf, cuda, lay, htf.optimizers.SGD(lr), 1)
        assert "generic" not in model.ops
        x = torch.from_numpy(tfc.get_nlist_array()).to(torch.float32).to(cuda)
        g = layer().wide_loss_gradient(x, tfc._labels[:sysm.N].contiguous(), model.index)[1:].double()
        return lay.w.double() - w0.double(), g, sysm.N

    _, g, N = run(1e-3)
    lr = 0.25 * 4 * N / g.abs().max().item()
    dw, g2, _ = run(lr)
    assert torch.equal(g2, g)
    want = -lr * g / (4 * N)
    err, scale = (dw - want).abs().max().item(), want.abs().max().item()
    print("one SGD step: lr %.4g, max|dw| %.3g, max err %.3g" % (lr, scale, err))
    assert err <= 1e-6 * scale
