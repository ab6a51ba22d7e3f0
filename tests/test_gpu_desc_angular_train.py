"""Force matching on the angular conservative forces of htf.DescriptorMLP on the MI355X (csrc/atrain.hip, include/htf_atrain.h;
DescriptorMLP.angular_loss_gradient, trainable="angular") against torch's fp64 double backward THROUGH THE POSITIONS of the
definition tests/test_gpu_desc_angular.py states:

    pred_i = (-d(sum_j E_j)/dr_i, E_i),  E_i = network([G | A | Q]_i),  SSR = sum_i |pred_i - labels_i|^2,
    accum = {SSR, d SSR / d theta}.

The systems are that module's jittered lattices (symmetric lists by geometry, exact fp32 pair vectors: it asserts both).  As for
the other two sweeps the reference is fed the sweep's own fp32 residual, labels_eff = ref_pred - (gpu_pred - labels).

Bound.  TOL = 2e-4 of the largest gradient entry is the project's bound for both existing sweeps, and the SSR to 1e-5.  A, Q and
their tangents are sums of products of partly cancelling moments, and what fp32 costs there is a property of the definition, not
of the kernel: every value test also evaluates the same reference with torch in fp32 (the twin) and allows max(TOL, 4 x the
twin's error), the rule and the factor of tests/test_gpu_desc_angular.py.  Both errors are printed before anything is asserted.

Lists that are not symmetric (cut short, indices outside the batch) are checked against the formula-level fp64 reference, which
takes the pair vectors as a leaf: Q = sum_is (rho_i - m_is rho_j) . dE_i/dx_is + sum_i rho_iE E_i, d SSR / d theta = 2 dQ/dtheta."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_desc_angular as A
import test_gpu_desc_total_train as TT
from test_gpu_desc_angular import _inputs, _layer, _neighbor_types, _system

pytestmark = pytest.mark.gpu
TOL = 2e-4


# ------------------------------------------------------------------------------------------------ the references
def angular_pred(lay, W, pos, L, idx, occ, tn, sp):
    """pred [N, 4] = (-grad(sum E, pos), E) in the dtype of ``pos`` and ``W``, differentiable in W."""
    q = pos.detach().clone().requires_grad_(True)
    X = _inputs(lay, A._pair_vectors(q, idx, occ, L), tn)[0]
    E = TT._net(lay, W, X, sp)
    (g,) = torch.autograd.grad(E.sum(), q, create_graph=True)
    return torch.cat([-g, E[:, None]], dim=1)


def reference_gradient(lay, p, L, x, idx, resid32, sp=None, dtype=torch.float64):
    """d SSR / d theta [S, P] by double backward through the positions, the residual being the sweep's own.  fp64 is the
    reference; dtype=torch.float32 is its twin, the same arithmetic at the kernel's precision."""
    sp = torch.zeros(len(p), dtype=torch.long, device=p.device) if sp is None else sp
    W = TT._weights(lay, p.device, dtype)
    occ = (x[:, :, :3] != 0).any(dim=2)
    pred = angular_pred(lay, W, p[:, :3].to(dtype), L, idx, occ, _neighbor_types(lay, x), sp)
    labels_eff = pred.detach() - resid32.to(dtype)
    return TT._flat(torch.autograd.grad(((pred - labels_eff) ** 2).sum(), W)).double()


def formula_gradient(lay, x, idx, resid32, sp=None, gather=True):
    """The formula-level fp64 reference on the tensor itself, for any list: the pair vectors are a leaf.  ``gather=False``:
    every m_is = 0."""
    B = x.shape[0]
    sp = torch.zeros(B, dtype=torch.long, device=x.device) if sp is None else sp
    W = TT._weights(lay, x.device)
    x3 = x[:, :, :3].double().detach().clone().requires_grad_(True)
    E = TT._net(lay, W, _inputs(lay, x3, _neighbor_types(lay, x))[0], sp)
    (gx,) = torch.autograd.grad(E.sum(), x3, create_graph=True)
    rho = resid32.double()
    d = rho[:, None, :3].expand(-1, x.shape[1], -1)
    if gather:
        j = idx.long()
        m = ((j >= 0) & (j < B)).to(torch.float64)
        d = d - rho[j.clamp(0, max(B - 1, 0)), :3] * m[..., None]
    Q = (gx * d).sum() + (rho[:, 3] * E).sum()
    return TT._flat(torch.autograd.grad(2.0 * Q, W)).double()


WORST = {}   # (l_max, "kernel" | "twin") -> the largest relative error seen in this run, printed by every check


def _check(lay, got, g, twin, ssr_got, ssr, what, blocks=True):
    """One network's accum[1:] against the fp64 gradient with the twin's error beside it, accum[0] against the fp64 SSR; prints
    every figure before it asserts."""
    got, g = got.double(), g.double()
    scale = g.abs().max().item()
    err = (got - g).abs().max().item() / scale
    tw = (twin.double() - g).abs().max().item() / scale if twin is not None else 0.0
    bound = max(TOL, 4.0 * tw)
    for key, val in (((lay.l_max, "kernel"), err), ((lay.l_max, "twin"), tw)):
        WORST[key] = max(WORST.get(key, 0.0), val)
    print("%s: kernel %.3g, fp32 twin %.3g of max|g| = %.3g; bound %.3g%s; SSR %.9g vs %.9g; worst so far %s"
          % (what, err, tw, scale, bound, " (ABOVE 2e-4)" if err > TOL else "", ssr_got, ssr, sorted(WORST.items())))
    for k, sl in TT._blocks(lay):
        print("   %s: max|g| = %.3g, max err = %.3g" % (k, g[sl].abs().max().item(), (got[sl] - g[sl]).abs().max().item()))
    assert np.isfinite(err) and scale > 0 and err <= bound, "%s: error %.3g over %.3g (twin %.3g)" % (what, err, bound, tw)
    assert abs(ssr_got - ssr) <= 1e-5 * ssr, (ssr_got, ssr)
    if blocks:
        for k, sl in TT._blocks(lay):
            assert g[sl].abs().max().item() > 0 and got[sl].abs().max().item() > 0, "%s carries no signal" % k


def _K(l_max, n_types):
    """K = 16 for one type (D = 32, 48); with three types the largest K with D <= 64: 10 (D = 60) and 7 (D = 63)."""
    return 16 if n_types == 1 else (10 if l_max == 1 else 7)


_labels = TT._labels


# ------------------------------------------------------------------------------------------------ 1. the gradient
@functools.lru_cache(maxsize=None)
def _case(l_max, config, n_types, activation, cut):
    """The layer of a case and a one-entry store for its references, shared by the tensor dtypes when the residual has the
    same bits."""
    import hoomd_tf_amd as htf
    rc_list = _system(config)[2]
    lay = _layer(htf, K=_K(l_max, n_types), n_types=n_types, activation=activation, high=rc_list,
                 r_cut=0.9 * rc_list if cut else None, seed=5 + n_types + 10 * l_max, H1=24, H2=20, l_max=l_max)
    return lay, {}


def _references(lay, store, p, L, x, idx, resid):
    if "resid" not in store or not torch.equal(store["resid"], resid):
        store["resid"] = resid.clone()
        store["g"] = reference_gradient(lay, p, L, x, idx, resid)[0]
        store["twin"] = reference_gradient(lay, p, L, x, idx, resid, dtype=torch.float32)[0]
    return store["g"], store["twin"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("activation", ["tanh", "linear"])
@pytest.mark.parametrize("n_types", [1, 3])
@pytest.mark.parametrize("config", ["a", "b256"])
@pytest.mark.parametrize("l_max", [1, 2])
def test_gradient_against_fp64_double_backward(htf, cuda, l_max, config, n_types, activation, cut, dtype):
    """K = 16 with one type, K = 10 (l_max 1) or 7 (l_max 2) with three (the system's types are 0, 1, 2); cutoff none or 0.9 of
    the list's."""
    p, L, rc_list, x, idx = _system(config)
    lay, store = _case(l_max, config, n_types, activation, cut)
    xx, types = x.to(dtype), p[:, 3].contiguous()
    labels = _labels(len(p), cuda, 7 + n_types)
    accum = lay.angular_loss_gradient(xx, labels, idx, types=types)
    assert accum.dtype == torch.float32 and accum.shape == (1 + lay.w.numel(),) and torch.isfinite(accum).all()
    pred = lay.total_forces(xx, idx, types=types).to(torch.float32)
    resid = pred - labels
    g, twin = _references(lay, store, p, L, x, idx, resid)
    _check(lay, accum[1:], g, twin, accum[0].item(), (resid.double() ** 2).sum().item(),
           "l_max=%d %s T=%d %s cut=%s %s" % (l_max, config, n_types, activation, cut, dtype))
    # a prediction handed in is the one evaluated inside
    assert torch.equal(lay.angular_loss_gradient(xx, labels, idx, pred=pred), accum)


# ------------------------------------------------------------------------------------------------ 2. the widest inputs
@pytest.mark.parametrize("K,n_types,l_max", [(32, 1, 1), (7, 3, 2)])
def test_widest_inputs(htf, cuda, K, n_types, l_max):
    """D = 64 and D = 63 with H1 = H2 = 64: every lane holds a network input and a hidden unit, no 16-row block of the
    accumulators is skipped, and the entries 2 Dr + c of the input lines are the last of the wave."""
    p, L, rc_list, x, idx = _system("a")
    lay = _layer(htf, K=K, n_types=n_types, high=rc_list, r_cut=0.9 * rc_list, seed=19 + l_max, H1=64, H2=64, l_max=l_max)
    assert lay.D == K * n_types * (1 + l_max) >= 63
    types, labels = p[:, 3].contiguous(), _labels(len(p), cuda, 20)
    accum = lay.angular_loss_gradient(x, labels, idx, types=types)
    resid = lay.total_forces(x, idx, types=types).to(torch.float32) - labels
    g = reference_gradient(lay, p, L, x, idx, resid)[0]
    twin = reference_gradient(lay, p, L, x, idx, resid, dtype=torch.float32)[0]
    _check(lay, accum[1:], g, twin, accum[0].item(), (resid.double() ** 2).sum().item(), "D = %d" % lay.D)


# ------------------------------------------------------------------------------------------------ 3. the angular terms
@pytest.mark.parametrize("l_max", [1, 2])
def test_angular_terms_are_there(htf, cuda, l_max):
    """With the A and Q rows of W1 non-zero, the radial rows of dW1 are not those of the l_max = 0 layer holding the same radial
    weights on the same residual: they differ by more than 100 x the bound, so a sweep that dropped vdot or Mdot (or fed the
    network G alone) cannot pass (1) on a weak case.  Each is within the bound of its own fp64 reference."""
    p, L, rc_list, x, idx = _system("a")
    lay = _layer(htf, K=16, high=rc_list, r_cut=0.9 * rc_list, seed=6, H1=24, H2=20, l_max=l_max)
    ws = lay.get_weights()
    ws[0][lay.Dr:2 * lay.Dr] *= np.float32(4.0)   # (A is a sum of cancelling vectors and small on a lattice: its rows can take it)
    lay.set_weights(ws)
    assert all(np.abs(ws[0][b * lay.Dr:(b + 1) * lay.Dr]).max() > 0 for b in range(1 + l_max))
    lay0 = htf.DescriptorMLP(K=16, H1=24, H2=20, low=0.5, high=rc_list, r_cut=0.9 * rc_list, conservative=True)
    lay0.set_weights([ws[0][:lay.Dr]] + ws[1:])
    labels = _labels(len(p), cuda, 8)
    pred = lay.total_forces(x, idx).to(torch.float32)
    resid = pred - labels
    got = lay.angular_loss_gradient(x, labels, idx, pred=pred)
    got0 = lay0.total_loss_gradient(x, labels, idx, pred=pred)   # (pred only forms the residual: the same one)
    g = reference_gradient(lay, p, L, x, idx, resid)[0]
    twin = reference_gradient(lay, p, L, x, idx, resid, dtype=torch.float32)[0]
    g0 = TT.reference_gradient(lay0, p, L, x, idx, resid)[0]
    _check(lay, got[1:], g, twin, got[0].item(), (resid.double() ** 2).sum().item(), "angular, l_max = %d" % l_max)
    n0 = lay.Dr * lay.H1
    err0, scale0 = (got0[1:].double() - g0).abs().max().item(), g0.abs().max().item()
    diff, scale = (got[1:1 + n0].double() - got0[1:1 + n0].double()).abs().max().item(), g.abs().max().item()
    print("radial rows of dW1: max|angular - radial| = %.3g of %.3g (ratio %.3g); the radial sweep's own error %.3g of %.3g"
          % (diff, scale, diff / scale, err0, scale0))
    assert err0 < TOL * scale0
    assert diff > 100 * TOL * scale


# ------------------------------------------------------------------------------------------------ 4. index outside [0, B)
@pytest.mark.parametrize("l_max", [1, 2])
def test_index_outside_the_batch(htf, cuda, l_max):
    """Every index -1, B or 2^31 - 1 and a zero energy residual: every m_is is 0, and the result is the formula-level reference
    without gathered residuals.  Nothing is read at those indices: the kernel compares the index with B as unsigned before it
    forms an address (csrc/atrain.hip, step 1), so there is nothing to probe here."""
    p, L, rc_list, x, idx = _system("a")
    B = len(p)
    lay = _layer(htf, K=_K(l_max, 3), n_types=3, high=rc_list, r_cut=0.9 * rc_list, seed=9, H1=24, H2=20, l_max=l_max)
    types = p[:, 3].contiguous()
    pred = lay.total_forces(x, idx, types=types).to(torch.float32)
    labels = pred.clone()
    labels[:, :3] += _labels(B, cuda, 10)[:, :3]
    resid = pred - labels
    assert (resid[:, 3] == 0).all()
    bad = torch.tensor([-1, B, 2 ** 31 - 1], dtype=torch.int32, device=cuda)[torch.arange(idx.numel(), device=cuda) % 3].view_as(idx).contiguous()
    got = lay.angular_loss_gradient(x, labels, bad, pred=pred)
    assert torch.isfinite(got).all()
    want = formula_gradient(lay, x, bad, resid, gather=False)[0]
    assert torch.equal(want, formula_gradient(lay, x, bad, resid)[0])   # (the reference's own m is 0 at every such index)
    _check(lay, got[1:], want, None, got[0].item(), (resid.double() ** 2).sum().item(), "index outside, l_max = %d" % l_max, blocks=False)
    # with the particles' own indices the answer is another: the gathered residuals are not small
    full = lay.angular_loss_gradient(x, labels, idx, pred=pred)[1:].double()
    assert (full - want).abs().max().item() > 100 * TOL * want.abs().max().item()


# ------------------------------------------------------------------------------------------------ 5. species
def test_one_network_per_species(htf, cuda):
    p, L, rc_list, x, idx = _system("a")
    B = len(p)
    lay = _layer(htf, K=7, n_types=3, high=rc_list, r_cut=0.9 * rc_list, n_species=2, seed=11, H1=24, H2=20, l_max=2)
    sp = torch.from_numpy(np.random.default_rng(12).integers(0, 2, B)).to(cuda)
    spf, types = sp.to(torch.float32), p[:, 3].contiguous()
    labels = _labels(B, cuda, 13)
    accum = lay.angular_loss_gradient(x, labels, idx, types=types, species=spf)
    assert accum.shape == (2, 1 + lay.P) and torch.isfinite(accum).all()
    resid = lay.total_forces(x, idx, types=types, species=spf).to(torch.float32) - labels
    g = reference_gradient(lay, p, L, x, idx, resid, sp=sp)
    twin = reference_gradient(lay, p, L, x, idx, resid, sp=sp, dtype=torch.float32)
    for s in range(2):
        _check(lay, accum[s, 1:], g[s], twin[s], accum[s, 0].item(), (resid[sp == s].double() ** 2).sum().item(), "species %d" % s)
    # every particle in species 1: network 0 has no rows
    ones = torch.ones(B, device=cuda)
    one = lay.angular_loss_gradient(x, labels, idx, types=types, species=ones)
    assert (one[0] == 0).all() and one[1, 1:].abs().max().item() > 0
    resid1 = lay.total_forces(x, idx, types=types, species=ones).to(torch.float32) - labels
    g1 = reference_gradient(lay, p, L, x, idx, resid1, sp=ones.long())
    t1 = reference_gradient(lay, p, L, x, idx, resid1, sp=ones.long(), dtype=torch.float32)
    assert (g1[0] == 0).all()
    _check(lay, one[1, 1:], g1[1], t1[1], one[1, 0].item(), (resid1.double() ** 2).sum().item(), "one species")


# ------------------------------------------------------------------------------------------------ 6. more rows than one grid pass
def test_more_rows_than_one_grid_pass(htf, cuda):
    """Config a's 216 rows tiled 152 times, the index shifted by 216 per tile: 32 832 rows, more than 512 x 64, so every one of
    the 512 partials is written and the grid-stride loop runs.  Reference: 152 x the single tile's fp64 gradient."""
    rep = 152
    p, L, rc_list, xa, idxa = _system("a")
    nb = len(p)
    lay = _layer(htf, K=16, high=rc_list, r_cut=0.9 * rc_list, seed=16, H1=24, H2=20, l_max=2)
    lb = _labels(nb, cuda, 17)
    x, labels = xa.repeat(rep, 1, 1).contiguous(), lb.repeat(rep, 1).contiguous()
    shift = (nb * torch.arange(rep, dtype=torch.int32, device=cuda)).repeat_interleave(nb)[:, None]
    idx = torch.where(idxa.repeat(rep, 1) >= 0, idxa.repeat(rep, 1) + shift, -1).to(torch.int32).contiguous()
    assert x.shape[0] == 32832 > 512 * 64
    pred_a = lay.total_forces(xa, idxa).to(torch.float32)
    pred = lay.total_forces(x, idx).to(torch.float32)
    assert torch.equal(pred[nb:2 * nb], pred_a) and torch.equal(pred[-nb:], pred_a)   # every tile is the block, bit for bit
    accum = lay.angular_loss_gradient(x, labels, idx, pred=pred)
    resid = pred_a - lb
    g = rep * reference_gradient(lay, p, L, xa, idxa, resid)[0]
    twin = rep * reference_gradient(lay, p, L, xa, idxa, resid, dtype=torch.float32)[0]
    _check(lay, accum[1:], g, twin, accum[0].item(), rep * (resid.double() ** 2).sum().item(), "tiled x %d" % rep)


# ------------------------------------------------------------------------------------------------ 7. bits
@pytest.mark.parametrize("l_max", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_bitwise_reproducible(htf, cuda, dtype, l_max):
    p, L, rc_list, x, idx = _system("b256")
    lay = _layer(htf, K=_K(l_max, 3), n_types=3, high=rc_list, r_cut=0.9 * rc_list, H1=64, H2=64, seed=14, l_max=l_max)
    xx, types, labels = x.to(dtype), p[:, 3].contiguous(), _labels(len(p), cuda, 15)
    a = lay.angular_loss_gradient(xx, labels, idx, types=types)
    b = lay.angular_loss_gradient(xx, labels, idx, types=types)
    assert torch.equal(a, b) and a[1:].abs().max().item() > 0
    out = torch.full_like(a, float("nan"))
    assert lay.angular_loss_gradient(xx, labels, idx, types=types, accum=out) is out and torch.equal(out, a)
    # a float index is taken by rint
    assert torch.equal(lay.angular_loss_gradient(xx, labels, idx.to(torch.float32) + 0.25, types=types), a)


@pytest.mark.parametrize("l_max", [1, 2])
def test_zero_rows(htf, cuda, l_max):
    lay = _layer(htf, K=8, n_types=2, l_max=l_max)
    for dt in (torch.float32, torch.float64):
        acc = lay.angular_loss_gradient(torch.zeros((0, 32, 4), dtype=dt, device=cuda), torch.zeros((0, 4), dtype=dt, device=cuda),
                                        torch.zeros((0, 32), dtype=torch.int32, device=cuda), types=torch.zeros((0,), device=cuda))
        assert acc.shape == (1 + lay.w.numel(),) and (acc == 0).all()


@pytest.mark.parametrize("NN", [1, 63, 64, 65, 128, 129])
def test_slot_counts(htf, cuda, NN):
    """The boundaries of the four-slots-per-lane layout, on config b256's list cut short (a list cut short is not symmetric: the
    formula-level reference takes any list).  Slot 0 is moved to the last slot, so that the last slot of every row is live."""
    p, L, rc_list, x, idx = _system("b256")
    x, idx = x[:, :NN].clone(), idx[:, :NN].clone()
    if NN > 1:
        x[:, -1], idx[:, -1] = x[:, 0].clone(), idx[:, 0].clone()
        x[:, 0], idx[:, 0] = 0.0, -1
    x, idx = x.contiguous(), idx.contiguous()
    lay = _layer(htf, K=10, n_types=2, high=rc_list, r_cut=0.9 * rc_list, seed=55, H1=24, H2=20, l_max=2)
    types, labels = p[:, 3].contiguous(), _labels(len(p), cuda, 56)
    pred = lay.total_forces(x, idx, types=types).to(torch.float32)
    resid = pred - labels
    got = lay.angular_loss_gradient(x, labels, idx, types=types, pred=pred)
    assert torch.isfinite(got).all()
    want = formula_gradient(lay, x, idx, resid)[0]
    _check(lay, got[1:], want, None, got[0].item(), (resid.double() ** 2).sum().item(), "NN = %d" % NN)


# ------------------------------------------------------------------------------------------------ 8. descent against torch twins
# chosen on the CPU (the same positions, a brute-force list): the fp64 twin's loss falls at every one of the 30 steps, from 0.345
# to 1.09e-2, so the rate of test_gpu_desc_total_train.py stands and was not lowered
DESCENT_LR = 3e-2


def descent_problem(htf, dev):
    """The student and the teacher whose total-energy forces label config a: the same shape, other weights.  The Q rows of W1
    are scaled as _layer scales them, so that tanh does not saturate."""
    kw = dict(K=16, H1=24, H2=20, low=0.5, high=1.8, r_cut=1.62, l_max=2)
    lay = htf.DescriptorMLP(seed=4, trainable="angular", device=dev, **kw)
    teacher = htf.DescriptorMLP(seed=17, conservative=True, device=dev, **kw)
    for m in (lay, teacher):
        ws = m.get_weights()
        ws[0][2 * m.Dr:] *= np.float32(1.0 / 64.0)
        m.set_weights(ws)
    return lay, teacher


def twin_descent(lay, pos, L, idx, occ, labels, dtype, lr, steps):
    """Plain SGD theta <- theta - lr g / (4 B) on SSR, the total-energy forces written in torch: (losses per step, final theta)."""
    W = TT._weights(lay, pos.device, dtype)
    q, ll = pos.to(dtype), labels.to(dtype)
    tn = torch.zeros(idx.shape, dtype=torch.float64, device=pos.device)
    sp = torch.zeros(len(pos), dtype=torch.long, device=pos.device)
    B, losses = len(pos), []
    for _ in range(steps):
        ssr = ((angular_pred(lay, W, q, L, idx, occ, tn, sp) - ll) ** 2).sum()
        gs = torch.autograd.grad(ssr, W)
        losses.append(ssr.item() / (4 * B))
        with torch.no_grad():
            for w, g in zip(W, gs):
                w -= lr * g / (4 * B)
    return losses, TT._flat([w.detach() for w in W])[0].double()


def test_descent_tracks_torch_twins(htf, cuda):
    """30 SGD steps on config a with l_max = 2 through angular_loss_gradient + ops.optimizer_step, beside the same forces and
    rule in torch fp64 and fp32; the labels are a teacher network's total-energy forces in fp64.  The kernel path's weights may
    leave the fp64 twin's by at most 4x what the fp32 twin's do."""
    from hoomd_tf_amd import ops
    steps = 30
    p, L, rc_list, x, idx = _system("a")
    pos, occ = p[:, :3].contiguous(), (x[:, :, :3] != 0).any(dim=2)
    lay, teacher = descent_problem(htf, cuda)
    tn = torch.zeros(idx.shape, dtype=torch.float64, device=cuda)
    sp = torch.zeros(len(p), dtype=torch.long, device=cuda)
    labels = angular_pred(teacher, TT._weights(teacher, cuda), pos, L, idx, occ, tn, sp).detach().to(torch.float32)
    l64, t64 = twin_descent(lay, pos, L, idx, occ, labels, torch.float64, DESCENT_LR, steps)
    l32, t32 = twin_descent(lay, pos, L, idx, occ, labels, torch.float32, DESCENT_LR, steps)
    print("descent: fp64 losses", ["%.4g" % v for v in l64])
    assert all(b < a for a, b in zip(l64, l64[1:])), l64
    state = torch.zeros(ops.optimizer_state_floats(lay.w.numel()), dtype=torch.float32, device=cuda)
    desc = htf.optimizers.SGD(DESCENT_LR).desc(lay.nonneg_mask, lay.l1_reg)
    B, losses = len(p), []
    for _ in range(steps):
        accum = lay.angular_loss_gradient(x, labels, idx)
        losses.append(accum[0].item() / (4 * B))
        ops.optimizer_step(lay.w, accum, 1.0 / (4 * B), state, desc)
    scale = t64.abs().max().item()
    dev32 = (t32 - t64).abs().max().item() / scale
    devk = (lay.w.double() - t64).abs().max().item() / scale
    print("descent: loss fp64 %.6g -> %.6g, fp32 twin %.6g -> %.6g, kernel %.6g -> %.6g" % (l64[0], l64[-1], l32[0], l32[-1], losses[0], losses[-1]))
    print("descent: max|theta - theta_fp64| / max|theta_fp64|: fp32 twin %.3g, kernel path %.3g" % (dev32, devk))
    assert losses[-1] < losses[0]
    assert abs(losses[0] - l64[0]) <= 1e-4 * l64[0]
    assert devk <= 4.0 * dev32, (devk, dev32)


# ------------------------------------------------------------------------------------------------ 9. through tfcompute
def _model(htf, lay):
    """test_gpu_desc_angular._model, keeping the step's own slot index as well."""
    class M(A._model(htf, lay)):
        def compute(self, nlist, positions, box):
            self.index = nlist.index   # (the step's own, built once: what the layer is about to read)
            return super().compute(nlist, positions, box)
    return M


def _training_run(htf, cuda, lay, optimizer, steps, batch_size=None, seed=23):
    """The fcc box of 500 particles of test_gpu_desc_angular._sim, LJ driving the run and labelling."""
    import build_examples
    sim, sysm, _ = A._sim(htf, cuda, seed)
    nlist = sim.nlist_cell()
    lj = htf.tfcompute(build_examples.LJModel(128))
    lj.attach(nlist, r_cut=2.5)
    model = _model(htf, lay)(128, output_forces=False)
    model.compile(optimizer, loss='MeanSquaredError')
    tfc = htf.tfcompute(model)
    tfc.attach(nlist, train=True, r_cut=2.5, batch_size=batch_size)
    tfc.set_reference_forces(lj)
    sim.run(steps)
    torch.cuda.synchronize()
    return model, tfc, sysm


def _tf_layer(htf):
    """fc vanishes before the list's cutoff 2.5: the step's list is symmetric within the descriptor's range."""
    return htf.DescriptorMLP(K=8, H1=8, H2=8, low=0.5, high=2.5, r_cut=2.0, l_max=2, trainable="angular")


def test_one_sgd_step_is_the_sweeps_gradient(htf, cuda):
    """After ONE SGD step from fresh weights, w - w0 = -lr g / (4 N), g from angular_loss_gradient on the step's own tensor, its
    index and its staged labels.  The step is sized as test_gpu_desc_total_train.py sizes its own: from a first, identical run,
    so that max|dw| is about 0.25 and fp32 weights of size ~0.5 are stored well inside the bound of 1e-6 max|dw|.  The loss
    metric is finite, and a second step runs."""
    def run(lr, steps=1):
        lay = _tf_layer(htf)
        assert lay.trainable == "angular" and lay.conservative
        w0 = lay.w.clone()
        model, tfc, sysm = _training_run(htf, cuda, lay, htf.optimizers.SGD(lr), steps)
        assert tfc._tplan is None and tfc._plan is None
        loss = float(model.metrics[0].result())
        assert np.isfinite(loss) and loss > 0
        x = torch.from_numpy(tfc.get_nlist_array()).to(torch.float32).to(cuda)
        fresh = _tf_layer(htf)
        assert torch.equal(fresh.w, w0) and x.shape[0] == sysm.N and model.index.shape == x.shape[:2]
        g = fresh.angular_loss_gradient(x, tfc._labels[:sysm.N].contiguous(), model.index)[1:].double()
        return lay.w.double() - w0.double(), g, sysm.N, loss

    _, g, N, _ = run(1e-3)
    lr = 0.25 * 4 * N / g.abs().max().item()
    dw, g2, _, loss = run(lr)
    assert torch.equal(g2, g)
    want = -lr * g / (4 * N)
    err, scale = (dw - want).abs().max().item(), want.abs().max().item()
    print("one SGD step: lr %.4g, max|dw| %.3g, max err %.3g (ratio %.3g), metric %.6g" % (lr, scale, err, err / scale, loss))
    assert err <= 1e-6 * scale
    # a second step runs on the stepped weights
    dw2, _, _, loss2 = run(1e-3, steps=2)
    assert torch.isfinite(dw2).all() and dw2.abs().max().item() > 0 and np.isfinite(loss2)


def test_batches_still_raise(htf, cuda):
    with pytest.raises(ValueError, match="batch"):
        _training_run(htf, cuda, _tf_layer(htf), htf.optimizers.Adam(0.01), 1, batch_size=500 // 3)
