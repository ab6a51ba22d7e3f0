"""Force matching on the conservative forces of htf.DescriptorMLP on the MI355X (csrc/ctrain.hip over dtrain_row.h,
include/htf_ctrain.h; DescriptorMLP.total_loss_gradient, trainable="total") against torch's fp64 double backward THROUGH THE
POSITIONS of the definition tests/test_gpu_desc_total.py states:

    pred_i = (-d(sum_j E_j)/dr_i, E_i),  SSR = sum_i |pred_i - labels_i|^2,  accum = {SSR, d SSR / d theta}.

The systems are that module's jittered lattices (symmetric lists by geometry, exact fp32 pair vectors: it asserts both).  As
for the row sweep (tests/test_gpu_desc_train.py) the reference is fed the sweep's own fp32 residual, labels_eff = ref_pred -
(gpu_pred - labels), and the bounds are that module's: 2e-4 of the largest gradient entry, the SSR to 1e-5."""
import math

import numpy as np
import pytest
import torch

import test_gpu_desc_total as T

pytestmark = pytest.mark.gpu
TOL = 2e-4
_KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")


# ------------------------------------------------------------------------------------------------ the fp64 reference
def _descriptor(lay, x3, tn):
    """G [B, D] of pair vectors x3 [B, NN, 3] and neighbor types tn [B, NN]: test_gpu_desc_total._descriptor in the dtype of x3."""
    mu = torch.as_tensor(lay.centers, dtype=x3.dtype, device=x3.device)
    t = x3 + 1e-7
    r = torch.sqrt((t * t).sum(dim=2))
    live = r > 3e-6
    fc = torch.ones_like(r)
    if lay.r_cut is not None:
        live = live & (r < lay.r_cut)
        fc = 0.5 * (torch.cos(math.pi * r / lay.r_cut) + 1.0)
    e = torch.exp(-(r[..., None] - mu) ** 2 / float(lay.gap)) * (fc * live.to(r.dtype))[..., None]
    return torch.cat([(e * (tn == tt).to(r.dtype)[..., None]).sum(dim=1) for tt in range(lay.n_types)], dim=1)


def _net(lay, W, G, sp):
    """test_gpu_desc_total._network on explicit weights W (six arrays with a leading species axis), differentiable in them."""
    act = torch.tanh if lay.activation == "tanh" else (lambda v: v)
    h1 = act(torch.einsum("bd,bdh->bh", G, W[0][sp]) + W[1][sp])
    h2 = act(torch.einsum("bd,bdh->bh", h1, W[2][sp]) + W[3][sp])
    return torch.einsum("bd,bdh->bh", h2, W[4][sp])[:, 0] + W[5][sp][:, 0]


def total_pred(lay, W, pos, L, idx, occ, tn, sp):
    """pred [N, 4] = (-grad(sum E, pos), E) in the dtype of ``pos`` and ``W``, differentiable in W."""
    q = pos.detach().clone().requires_grad_(True)
    G = _descriptor(lay, T._pair_vectors(q, idx, occ, L), tn)
    E = _net(lay, W, G, sp)
    (g,) = torch.autograd.grad(E.sum(), q, create_graph=True)
    return torch.cat([-g, E[:, None]], dim=1)


def _weights(lay, dev, dtype=torch.float64):
    W = [torch.as_tensor(np.asarray(w), device=dev).to(dtype) for w in lay.get_weights()]
    return [(w if lay.n_species > 1 else w[None]).clone().requires_grad_(True) for w in W]


def _flat(gs):
    """Six arrays [S, ...] -> [S, P] in the order of the layer's flat weights."""
    return torch.cat([g.reshape(g.shape[0], -1) for g in gs], dim=1)


def reference_gradient(lay, p, L, x, idx, resid32, sp=None):
    """d SSR / d theta [S, P] in fp64 by double backward through the positions, the residual being the sweep's own."""
    sp = torch.zeros(len(p), dtype=torch.long, device=p.device) if sp is None else sp
    W = _weights(lay, p.device)
    occ = (x[:, :, :3] != 0).any(dim=2)
    pred = total_pred(lay, W, p[:, :3], L, idx, occ, T._neighbor_types(lay, x), sp)
    labels_eff = pred.detach() - resid32.double()
    return _flat(torch.autograd.grad(((pred - labels_eff) ** 2).sum(), W))


def _blocks(lay):
    o = 0
    for k, shape in zip(_KEYS, lay._shapes):
        n = int(np.prod(shape))
        yield k, slice(o, o + n)
        o += n


def _check(lay, got, g, ssr_got, ssr, what):
    """One network's accum[1:] against the fp64 gradient, accum[0] against the fp64 SSR; prints each figure before it asserts."""
    got, g = got.double(), g.double()
    scale, err = g.abs().max().item(), (got - g).abs().max().item()
    print("%s: max|got - g| = %.3g, max|g| = %.3g, ratio %.3g; SSR %.9g vs %.9g" % (what, err, scale, err / scale, ssr_got, ssr))
    for k, sl in _blocks(lay):
        print("   %s: max|g| = %.3g, max err = %.3g" % (k, g[sl].abs().max().item(), (got[sl] - g[sl]).abs().max().item()))
    assert np.isfinite(err) and scale > 0 and err < TOL * scale, "%s: max err %.3g of scale %.3g" % (what, err, scale)
    assert abs(ssr_got - ssr) <= 1e-5 * ssr, (ssr_got, ssr)
    for k, sl in _blocks(lay):
        assert g[sl].abs().max().item() > 0 and got[sl].abs().max().item() > 0, "%s carries no signal" % k


def _layer(htf, **kw):
    kw.setdefault("H1", 24)
    kw.setdefault("H2", 20)
    return T._layer(htf, **kw)


def _labels(B, cuda, seed):
    return torch.from_numpy(0.05 * np.random.default_rng(seed).standard_normal((B, 4))).to(torch.float32).to(cuda)


# ------------------------------------------------------------------------------------------------ 1. the gradient
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("activation", ["tanh", "linear"])
@pytest.mark.parametrize("n_types", [1, 3])
@pytest.mark.parametrize("config", ["a", "b", "b256"])
def test_gradient_against_fp64_double_backward(htf, cuda, config, n_types, activation, cut, dtype):
    """K = 16 with one type, K = 10 with three (the system's types are 0, 1, 2); cutoff none or 0.9 of the list's."""
    p, L, rc_list, x, idx = T._system(config)
    lay = _layer(htf, K=16 if n_types == 1 else 10, n_types=n_types, activation=activation, high=rc_list,
                 r_cut=0.9 * rc_list if cut else None, seed=5 + n_types)
    xx, types = x.to(dtype), p[:, 3].contiguous()
    labels = _labels(len(p), cuda, 7 + n_types)
    accum = lay.total_loss_gradient(xx, labels, idx, types=types)
    assert accum.dtype == torch.float32 and accum.shape == (1 + lay.w.numel(),) and torch.isfinite(accum).all()
    pred = lay.total_forces(xx, idx, types=types).to(torch.float32)
    resid = pred - labels
    g = reference_gradient(lay, p, L, x, idx, resid)[0]
    _check(lay, accum[1:], g, accum[0].item(), (resid.double() ** 2).sum().item(),
           "%s T=%d %s cut=%s %s" % (config, n_types, activation, cut, dtype))
    # a prediction handed in is the one evaluated inside
    assert torch.equal(lay.total_loss_gradient(xx, labels, idx, pred=pred), accum)


# ------------------------------------------------------------------------------------------------ 2. the reverse term
def test_reverse_term_is_there(htf, cuda):
    """The gradient of the fit to the total-energy forces is not the row operator's on the same residual: they differ by more
    than 100 x the bound of (1), so a sweep that forgot rho_j cannot pass (1) on a weak case."""
    p, L, rc_list, x, idx = T._system("a")
    lay = _layer(htf, K=16, high=rc_list, r_cut=0.9 * rc_list, seed=6)
    labels = _labels(len(p), cuda, 8)
    pred = lay.total_forces(x, idx).to(torch.float32)
    g = reference_gradient(lay, p, L, x, idx, pred - labels)[0]
    row = lay.loss_gradient(x, labels, pred=pred)[1:].double()
    diff, scale = (row - g).abs().max().item(), g.abs().max().item()
    print("reverse term: max|row sweep - g| = %.3g, max|g| = %.3g, ratio %.3g" % (diff, scale, diff / scale))
    assert diff > 100 * TOL * scale
    got = lay.total_loss_gradient(x, labels, idx, pred=pred)[1:].double()
    assert (got - g).abs().max().item() < TOL * scale


# ------------------------------------------------------------------------------------------------ 3. index outside [0, B)
def test_index_outside_the_batch(htf, cuda):
    """Every index -1, B or 2^31 - 1 and a zero energy residual: every m_is is 0 and a is half the row sweep's, so accum[1:] is
    0.5 loss_gradient(...)[1:] on the same force residual.  Nothing is read at those indices."""
    p, L, rc_list, x, idx = T._system("a")
    B = len(p)
    lay = _layer(htf, K=10, n_types=3, high=rc_list, r_cut=0.9 * rc_list, seed=9)
    pred = lay.forces(x).to(torch.float32)
    labels = pred.clone()
    labels[:, :3] += _labels(B, cuda, 10)[:, :3]
    assert ((pred - labels)[:, 3] == 0).all()
    bad = torch.tensor([-1, B, 2 ** 31 - 1], dtype=torch.int32, device=cuda)[torch.arange(idx.numel(), device=cuda) % 3].view_as(idx).contiguous()
    got = lay.total_loss_gradient(x, labels, bad, pred=pred)
    row = lay.loss_gradient(x, labels, pred=pred)
    assert torch.isfinite(got).all()
    want = 0.5 * row[1:].double()
    err, scale = (got[1:].double() - want).abs().max().item(), want.abs().max().item()
    print("index outside: max|got - row / 2| = %.3g of %.3g (equal bits: %s); SSR %.9g vs %.9g"
          % (err, scale, torch.equal(got[1:], 0.5 * row[1:]), got[0].item(), row[0].item()))
    assert scale > 0 and err < TOL * scale
    assert abs(got[0].item() - row[0].item()) <= 1e-5 * row[0].item()
    # with the particles' own indices the answer is another: the reverse terms are not small
    full = lay.total_loss_gradient(x, labels, idx, pred=pred)[1:].double()
    assert (full - want).abs().max().item() > 100 * TOL * scale


# ------------------------------------------------------------------------------------------------ 4. species
def test_one_network_per_species(htf, cuda):
    p, L, rc_list, x, idx = T._system("a")
    B = len(p)
    lay = _layer(htf, K=10, n_types=3, high=rc_list, r_cut=0.9 * rc_list, n_species=2, seed=11)
    sp = torch.from_numpy(np.random.default_rng(12).integers(0, 2, B)).to(cuda)
    spf, types = sp.to(torch.float32), p[:, 3].contiguous()
    labels = _labels(B, cuda, 13)
    accum = lay.total_loss_gradient(x, labels, idx, types=types, species=spf)
    assert accum.shape == (2, 1 + lay.P) and torch.isfinite(accum).all()
    pred = lay.total_forces(x, idx, types=types, species=spf).to(torch.float32)
    resid = pred - labels
    g = reference_gradient(lay, p, L, x, idx, resid, sp=sp)
    for s in range(2):
        _check(lay, accum[s, 1:], g[s], accum[s, 0].item(), (resid[sp == s].double() ** 2).sum().item(), "species %d" % s)
    # every particle in species 1: network 0 has no rows
    ones = torch.ones(B, device=cuda)
    one = lay.total_loss_gradient(x, labels, idx, types=types, species=ones)
    assert (one[0] == 0).all() and one[1, 1:].abs().max().item() > 0
    resid1 = lay.total_forces(x, idx, types=types, species=ones).to(torch.float32) - labels
    g1 = reference_gradient(lay, p, L, x, idx, resid1, sp=ones.long())
    assert (g1[0] == 0).all()
    _check(lay, one[1, 1:], g1[1], one[1, 0].item(), (resid1.double() ** 2).sum().item(), "one species")


# ------------------------------------------------------------------------------------------------ 5. reproducibility
def test_bitwise_reproducible(htf, cuda):
    p, L, rc_list, x, idx = T._system("b")
    lay = _layer(htf, K=16, high=rc_list, r_cut=0.9 * rc_list, H1=64, H2=64, seed=14)
    labels = _labels(len(p), cuda, 15)
    a = lay.total_loss_gradient(x, labels, idx)
    b = lay.total_loss_gradient(x, labels, idx)
    assert torch.equal(a, b) and a[1:].abs().max().item() > 0
    out = torch.full_like(a, float("nan"))
    assert lay.total_loss_gradient(x, labels, idx, accum=out) is out and torch.equal(out, a)
    # a float index is taken by rint
    assert torch.equal(lay.total_loss_gradient(x, labels, idx.to(torch.float32) + 0.25), a)


def test_zero_rows(htf, cuda):
    lay = _layer(htf, K=8, n_types=2)
    for dt in (torch.float32, torch.float64):
        acc = lay.total_loss_gradient(torch.zeros((0, 32, 4), dtype=dt, device=cuda), torch.zeros((0, 4), dtype=dt, device=cuda),
                                      torch.zeros((0, 32), dtype=torch.int32, device=cuda), types=torch.zeros((0,), device=cuda))
        assert acc.shape == (1 + lay.w.numel(),) and (acc == 0).all()


# ------------------------------------------------------------------------------------------------ 6. more than 512 partials
def test_more_partials_than_the_reduction_has_blocks(htf, cuda):
    """Config b's 343 rows tiled 100 times, the index shifted by 343 per tile: 34 300 rows, more than 512 x 64, so every block
    takes several rounds of rows and all 512 partials take part.  Reference: 100 x the block's fp64 gradient."""
    rep = 100
    p, L, rc_list, xb, idxb = T._system("b")
    nb = len(p)
    lay = _layer(htf, K=16, high=rc_list, r_cut=0.9 * rc_list, seed=16)
    lb = _labels(nb, cuda, 17)
    x, labels = xb.repeat(rep, 1, 1).contiguous(), lb.repeat(rep, 1).contiguous()
    shift = (nb * torch.arange(rep, dtype=torch.int32, device=cuda)).repeat_interleave(nb)[:, None]
    idx = torch.where(idxb.repeat(rep, 1) >= 0, idxb.repeat(rep, 1) + shift, -1).to(torch.int32).contiguous()
    assert x.shape[0] == 34300 > 512 * 64
    pred_b = lay.total_forces(xb, idxb).to(torch.float32)
    assert torch.equal(lay.total_forces(x, idx)[nb:2 * nb], pred_b)   # every tile is the block, bit for bit: so is its residual
    accum = lay.total_loss_gradient(x, labels, idx)
    g = rep * reference_gradient(lay, p, L, xb, idxb, pred_b - lb)[0]
    _check(lay, accum[1:], g, accum[0].item(), rep * ((pred_b - lb).double() ** 2).sum().item(), "tiled x %d" % rep)


# ------------------------------------------------------------------------------------------------ 7. descent against torch twins
# chosen on the CPU (the same positions, a brute-force list): the fp64 twin's loss falls at every one of the 30 steps, from 1.92
# to 1.7e-3 (it still does at 0.1, not at 0.3)
DESCENT_LR = 3e-2


def descent_problem(htf, dev):
    """The student and the teacher whose total-energy forces label config a: the same shape, other weights."""
    kw = dict(K=16, H1=24, H2=20, low=0.5, high=1.8, r_cut=1.62)
    lay = htf.DescriptorMLP(seed=4, trainable="total", device=dev, **kw)
    teacher = htf.DescriptorMLP(seed=17, device=dev, **kw)
    return lay, teacher


def twin_descent(lay, pos, L, idx, occ, labels, dtype, lr, steps):
    """Plain SGD theta <- theta - lr g / (4 B) on SSR, the total-energy forces written in torch: (losses per step, final theta)."""
    W = _weights(lay, pos.device, dtype)
    q, ll = pos.to(dtype), labels.to(dtype)
    tn = torch.zeros(idx.shape, dtype=dtype, device=pos.device)
    sp = torch.zeros(len(pos), dtype=torch.long, device=pos.device)
    B, losses = len(pos), []
    for _ in range(steps):
        ssr = ((total_pred(lay, W, q, L, idx, occ, tn, sp) - ll) ** 2).sum()
        gs = torch.autograd.grad(ssr, W)
        losses.append(ssr.item() / (4 * B))
        with torch.no_grad():
            for w, g in zip(W, gs):
                w -= lr * g / (4 * B)
    return losses, _flat([w.detach() for w in W])[0].double()


def test_descent_tracks_torch_twins(htf, cuda):
    """30 SGD steps on config a through total_loss_gradient + ops.optimizer_step, beside the same forces and rule in torch
    fp64 and fp32; the labels are a teacher network's total-energy forces in fp64.  The kernel path's weights may leave the
    fp64 twin's by at most 4x what the fp32 twin's do (the margin of test_gpu_desc_train.py's descent test)."""
    from hoomd_tf_amd import ops
    steps = 30
    p, L, rc_list, x, idx = T._system("a")
    pos, occ = p[:, :3].contiguous(), (x[:, :, :3] != 0).any(dim=2)
    lay, teacher = descent_problem(htf, cuda)
    tn = torch.zeros(idx.shape, dtype=torch.float64, device=cuda)
    sp = torch.zeros(len(p), dtype=torch.long, device=cuda)
    labels = total_pred(teacher, _weights(teacher, cuda), pos, L, idx, occ, tn, sp).detach().to(torch.float32)
    l64, t64 = twin_descent(lay, pos, L, idx, occ, labels, torch.float64, DESCENT_LR, steps)
    l32, t32 = twin_descent(lay, pos, L, idx, occ, labels, torch.float32, DESCENT_LR, steps)
    assert all(b < a for a, b in zip(l64, l64[1:])), l64
    state = torch.zeros(ops.optimizer_state_floats(lay.w.numel()), dtype=torch.float32, device=cuda)
    desc = htf.optimizers.SGD(DESCENT_LR).desc(lay.nonneg_mask, lay.l1_reg)
    B, losses = len(p), []
    for _ in range(steps):
        accum = lay.total_loss_gradient(x, labels, idx)
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


# ------------------------------------------------------------------------------------------------ 8. through tfcompute
def _model(htf, lay):
    class M(htf.SimModel):
        def setup(self):
            self.desc = lay
            self.ops = []
            self.index = None

        def compute(self, nlist, positions, box):
            log = htf.simmodel._trace_log()
            mark = len(log)
            out = htf.compute_nlist_forces(nlist, self.desc(nlist))
            self.ops.extend(e.get("op") for e in log[mark:])
            self.index = nlist.index   # (the step's own, built once: what the layer has just read)
            return out
    return M


def _training_run(htf, cuda, lay, optimizer, steps, batch_size=None, seed=23):
    """test_gpu_desc_train.py::_training_run with the model above: the fcc box of 500 particles, LJ driving the run and labelling."""
    import build_examples
    from test_gpu_desc_train import _fcc_sim
    sim, sysm = _fcc_sim(htf, cuda, seed=seed)
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
    return htf.DescriptorMLP(K=8, H1=8, H2=8, low=0.5, high=2.5, r_cut=2.0, trainable="total")


def test_training_through_tfcompute(htf, cuda):
    lay = _tf_layer(htf)
    assert lay.trainable == "total" and lay.conservative
    w0 = lay.w.clone()
    model, tfc, sysm = _training_run(htf, cuda, lay, htf.optimizers.Adam(0.01), 30)
    assert tfc._tplan is None and tfc._plan is None and tfc._train_seen is None
    assert "generic" not in model.ops and model.ops.count("descriptor_mlp") >= 30
    assert torch.isfinite(lay.w).all() and (lay.w - w0).abs().max().item() > 1e-3
    loss = float(model.metrics[0].result())
    print("tfcompute: |dw| max %.3g, metric %.6g, last loss %.6g" % ((lay.w - w0).abs().max().item(), loss, float(tfc._opt_state[20])))
    assert np.isfinite(loss) and loss > 0


def test_one_sgd_step_is_the_sweeps_gradient(htf, cuda):
    """After ONE SGD step from fresh weights, w - w0 = -lr g / (4 N), g from total_loss_gradient on the step's own tensor, its
    index and its staged labels.  The step is sized as test_gpu_desc_train.py sizes its own: from a first, identical run, so
    that max|dw| is about 0.25 and fp32 weights of size ~0.5 are stored well inside the bound of 1e-6 max|dw|."""
    def run(lr):
        lay = _tf_layer(htf)
        w0 = lay.w.clone()
        model, tfc, sysm = _training_run(htf, cuda, lay, htf.optimizers.SGD(lr), 1)
        x = torch.from_numpy(tfc.get_nlist_array()).to(torch.float32).to(cuda)
        fresh = _tf_layer(htf)
        assert torch.equal(fresh.w, w0) and x.shape[0] == sysm.N and model.index.shape == x.shape[:2]
        g = fresh.total_loss_gradient(x, tfc._labels[:sysm.N].contiguous(), model.index)[1:].double()
        return lay.w.double() - w0.double(), g, sysm.N

    _, g, N = run(1e-3)
    lr = 0.25 * 4 * N / g.abs().max().item()
    dw, g2, _ = run(lr)
    assert torch.equal(g2, g)
    want = -lr * g / (4 * N)
    err, scale = (dw - want).abs().max().item(), want.abs().max().item()
    print("one SGD step: lr %.4g, max|dw| %.3g, max err %.3g" % (lr, scale, err))
    assert err <= 1e-6 * scale


def test_batches_still_raise(htf, cuda):
    with pytest.raises(ValueError, match="batch"):
        _training_run(htf, cuda, _tf_layer(htf), htf.optimizers.Adam(0.01), 1, batch_size=500 // 3)
