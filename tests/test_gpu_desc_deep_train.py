"""Force matching for three hidden layers on the MI355X (csrc/cfw3train.hip, include/htf_cfw3train.h;
DescriptorMLP.deep_loss_gradient, trainable="deep") against the reference of test_gpu_desc_total_train.py with a three-layer
network: torch's fp64 double backward through the positions, fed the sweep's own fp32 residual.  Systems are
test_gpu_desc_total.py's, layers test_gpu_desc_deep.py's; every row count (216, 343) is ragged against the tiles of 32 and 16.

Bound: accum[0] to 1e-5 of the fp64 SSR, and the largest gradient error below 2e-4 sqrt(max(H1, H2, H3, 64) / 64) of the largest
reference entry -- test_gpu_desc_wide_train.py's rule with the third width.

Largest error / largest reference entry measured per case of test_gradient_against_fp64_double_backward, in CASES' order:
9.4e-8, 7.5e-8, 1.1e-7, 2.9e-7, 9.0e-8, 1.8e-7, 2.5e-7, 1.2e-7, 9.3e-8, 8.6e-8, 1.8e-7; species 4.9e-8 and 6.2e-8; tiled 1.8e-7."""
import math

import numpy as np
import pytest
import torch

import test_gpu_desc_total_train as TT
from test_gpu_desc_deep import _deep
from test_gpu_desc_total import _system
from test_gpu_desc_total_train import _labels, _training_run, reference_gradient

pytestmark = pytest.mark.gpu
CAP = 256   # include/htf_cfw3train.h HTF_CFW3T_MAX_BLOCKS: the launcher's grid cap, one block per tile below it


def _net3(lay, W, G, sp):
    """test_gpu_desc_total_train._net with the third hidden layer (eight arrays with a leading species axis)."""
    act = torch.tanh if lay.activation == "tanh" else (lambda v: v)
    h = G
    for i in (0, 2, 4):
        h = act(torch.einsum("bd,bdh->bh", h, W[i][sp]) + W[i + 1][sp])
    return torch.einsum("bd,bdh->bh", h, W[6][sp])[:, 0] + W[7][sp][:, 0]


@pytest.fixture(autouse=True)
def _three_layers(monkeypatch):
    monkeypatch.setattr(TT, "_net", _net3)


def _case(htf, cuda, config, seed, H1, H2, H3, cut=True, **kw):
    p, L, rc_list, x, idx = _system(config)
    assert len(p) % 32 and len(p) % 16
    lay = _deep(htf, H1, H2, H3, high=rc_list, r_cut=0.9 * rc_list if cut else None, seed=seed, **kw)
    return p, L, x, idx, p[:, 3].contiguous(), lay, _labels(len(p), cuda, seed + 2)


def _check(lay, got, g, ssr_got, ssr, what):
    """TT._check for eight weight blocks and the bound of the module docstring; prints each figure before it asserts."""
    got, g = got.double(), g.double()
    tol = 2e-4 * math.sqrt(max(lay.H1, lay.H2, lay.H3, 64) / 64.0)
    scale, err = g.abs().max().item(), (got - g).abs().max().item()
    print("%s: max|got - g| = %.3g, max|g| = %.3g, ratio %.3g; SSR %.9g vs %.9g" % (what, err, scale, err / scale, ssr_got, ssr))
    assert np.isfinite(err) and scale > 0 and err < tol * scale, "%s: max err %.3g of scale %.3g" % (what, err, scale)
    assert abs(ssr_got - ssr) <= 1e-5 * ssr, (ssr_got, ssr)
    o = 0
    for k, shape in zip(lay._KEYS, lay._shapes):
        sl = slice(o, o + int(np.prod(shape)))
        o = sl.stop
        assert g[sl].abs().max().item() > 0 and got[sl].abs().max().item() > 0, "%s carries no signal" % k
    assert o == lay.P and len(lay._KEYS) == 8


# (H1, H2, H3, config, K, n_types, cut, activation, dtype).  The tile: 16 rows at 256^3, 240^3 and 64 x 256 x 224 x 96 (640 image
# lines), 32 rows at all others; 64 x 256 x 192 x 96 (608 lines) is the widest the 32-row tile takes.  D = 16, 21 and 64.
CASES = [
    (256, 256, 256, "b256", 16, 4, True, "tanh", torch.float32),
    (256, 256, 256, "a", 7, 3, False, "linear", torch.float64),
    (240, 240, 240, "b", 16, 1, True, "tanh", torch.float64),
    (160, 128, 96, "b256", 16, 4, False, "tanh", torch.float32),
    (256, 192, 96, "a", 16, 4, True, "tanh", torch.float32),
    (256, 224, 96, "a", 16, 4, False, "tanh", torch.float64),
    (65, 33, 97, "a", 7, 3, False, "tanh", torch.float32),
    (65, 33, 97, "b256", 16, 1, True, "linear", torch.float64),
    (8, 256, 8, "a", 16, 4, True, "tanh", torch.float32),
    (32, 24, 16, "b", 7, 3, False, "linear", torch.float32),
    (1, 1, 1, "a", 16, 1, True, "tanh", torch.float64),
]


@pytest.mark.parametrize("H1,H2,H3,config,K,n_types,cut,activation,dtype", CASES)
def test_gradient_against_fp64_double_backward(htf, cuda, H1, H2, H3, config, K, n_types, cut, activation, dtype):
    p, L, x, idx, types, lay, labels = _case(htf, cuda, config, 5 + n_types, H1, H2, H3, cut=cut, K=K, n_types=n_types,
                                             activation=activation)
    xx = x.to(dtype)
    accum = lay.deep_loss_gradient(xx, labels, idx, types=types)
    assert accum.dtype == torch.float32 and accum.shape == (1 + lay.P,) and torch.isfinite(accum).all()
    resid = lay.total_forces(xx, idx, types=types).to(torch.float32) - labels
    g = reference_gradient(lay, p, L, x, idx, resid)[0]
    _check(lay, accum[1:], g, accum[0].item(), (resid.double() ** 2).sum().item(),
           "%d x %d x %d %s D=%d %s cut=%s %s" % (H1, H2, H3, config, K * n_types, activation, cut, dtype))


def test_one_network_per_species(htf, cuda):
    p, L, x, idx, types, lay, labels = _case(htf, cuda, "a", 11, 96, 160, 40, K=20, n_types=2, n_species=3)
    sp = (p[:, 3].long() % 2) * 2   # species 1 is absent
    spf = sp.to(torch.float32)
    accum = lay.deep_loss_gradient(x, labels, idx, types=types, species=spf)
    assert accum.shape == (3, 1 + lay.P) and (accum[1] == 0).all()
    resid = lay.total_forces(x, idx, types=types, species=spf).to(torch.float32) - labels
    g = reference_gradient(lay, p, L, x, idx, resid, sp=sp)
    for s in (0, 2):
        _check(lay, accum[s, 1:], g[s], accum[s, 0].item(), (resid[sp == s].double() ** 2).sum().item(), "species %d" % s)


def test_more_tiles_than_blocks(htf, cuda):
    """Config b's 343 rows 48 times, the index shifted by 343 per copy: 16 464 rows > 2 x 32 x CAP, 515 tiles on CAP blocks, so
    every block adds at least a second tile into its partial.  Reference: 48 x the block's fp64 gradient."""
    rep = 48
    p, L, xb, idxb, types, lay, lb = _case(htf, cuda, "b", 16, 32, 24, 16)
    nb = len(p)
    x, labels = xb.repeat(rep, 1, 1).contiguous(), lb.repeat(rep, 1).contiguous()
    shift = (nb * torch.arange(rep, dtype=torch.int32, device=cuda)).repeat_interleave(nb)[:, None]
    idx = torch.where(idxb.repeat(rep, 1) >= 0, idxb.repeat(rep, 1) + shift, -1).to(torch.int32).contiguous()
    assert x.shape[0] > 2 * 32 * CAP
    pred_b = lay.total_forces(xb, idxb).to(torch.float32)
    accum = lay.deep_loss_gradient(x, labels, idx, pred=pred_b.repeat(rep, 1).contiguous())
    g = rep * reference_gradient(lay, p, L, xb, idxb, pred_b - lb)[0]
    _check(lay, accum[1:], g, accum[0].item(), rep * ((pred_b - lb).double() ** 2).sum().item(), "tiled x %d" % rep)


def test_bits_and_edges(htf, cuda):
    p, L, x, idx, types, lay, labels = _case(htf, cuda, "b", 14, 256, 256, 256)
    a = lay.deep_loss_gradient(x, labels, idx)
    assert torch.equal(lay.deep_loss_gradient(x, labels, idx), a) and a[1:].abs().max().item() > 0
    out = torch.full_like(a, float("nan"))
    assert lay.deep_loss_gradient(x, labels, idx, accum=out) is out and torch.equal(out, a)
    pred = lay.total_forces(x, idx).to(torch.float32)
    assert torch.equal(lay.deep_loss_gradient(x, labels, idx, pred=pred), a)   # a prediction handed in is the one evaluated
    assert not torch.equal(lay.deep_loss_gradient(x, labels, idx, pred=pred + 0.01), a)
    for dt in (torch.float32, torch.float64):
        acc = lay.deep_loss_gradient(torch.zeros((0, 32, 4), dtype=dt, device=cuda), torch.zeros((0, 4), dtype=dt, device=cuda),
                                     torch.zeros((0, 32), dtype=torch.int32, device=cuda))
        assert acc.shape == (1 + lay.P,) and (acc == 0).all()


def test_one_sgd_step_through_tfcompute(htf, cuda):
    """After ONE SGD step from fresh weights, w - w0 = -lr g / (4 N), g from deep_loss_gradient on the step's own tensor, index
    and labels; the step is sized from a first, identical run, as test_gpu_desc_wide_train.py sizes its own."""
    def layer():
        return htf.DescriptorMLP(K=8, H1=96, H2=80, H3=40, low=0.5, high=2.5, r_cut=2.0, trainable="deep")

    def run(lr):
        lay = layer()
        w0 = lay.w.clone()
        model, tfc, sysm = _training_run(htf, cuda, lay, htf.optimizers.SGD(lr), 1)
        assert "generic" not in model.ops
        x = torch.from_numpy(tfc.get_nlist_array()).to(torch.float32).to(cuda)
        g = layer().deep_loss_gradient(x, tfc._labels[:sysm.N].contiguous(), model.index)[1:].double()
        return lay.w.double() - w0.double(), g, sysm.N

    _, g, N = run(1e-3)
    lr = 0.25 * 4 * N / g.abs().max().item()
    dw, g2, _ = run(lr)
    assert torch.equal(g2, g)
    want = -lr * g / (4 * N)
    err, scale = (dw - want).abs().max().item(), want.abs().max().item()
    print("one SGD step: lr %.4g, max|dw| %.3g, max err %.3g" % (lr, scale, err))
    assert err <= 1e-6 * scale
