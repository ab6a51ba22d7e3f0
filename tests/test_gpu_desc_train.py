"""Force matching for htf.DescriptorMLP on the MI355X (csrc/bp.hip over dtrain_row.h) against torch's fp64 double backward of the layer's
definition (the reference() construction of tests/test_gpu_desc.py, made differentiable in the weights):

    pred_i = (F_i, E_i),  SSR = sum_i |pred_i - labels_i|^2,  accum = {SSR, d SSR / d theta},  theta = W1|b1|W2|b2|W3|b3.

As for the project's other training sweeps (tests/test_gpu_training.py) the reference is fed the sweep's own fp32 residual,
labels_eff = ref_pred - (gpu_pred - labels), so that the bound, 2e-4 of the largest gradient entry, does not depend on how
large the residual is."""
import numpy as np
import pytest
import torch

from helpers import random_nlist

pytestmark = pytest.mark.gpu
TOL = 2e-4
_KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")


def _layer(htf, K=16, n_types=1, H1=24, H2=20, activation="tanh", low=0.0, high=3.0, seed=3, bias=0.1, trainable=True):
    lay = htf.DescriptorMLP(K=K, H1=H1, H2=H2, low=low, high=high, n_types=n_types, activation=activation, seed=seed,
                            trainable=trainable)
    if bias:   # (mlp_params' zero biases would leave the bias paths untested)
        rng = np.random.default_rng(seed + 100)
        ws = lay.get_weights()
        for i in (1, 3, 5):
            ws[i] = (bias * rng.standard_normal(ws[i].shape)).astype(np.float32)
        lay.set_weights(ws)
    return lay


def net(lay, W, x):
    """The layer's definition in plain torch, in the dtype of ``x`` and ``W`` (the six Keras arrays), differentiable in
    ``W``: pred [B, 4] = (2 sum_j dE_i/dx_ij, E_i)."""
    mu = torch.as_tensor(lay.centers, dtype=x.dtype, device=x.device)
    act = torch.tanh if lay.activation == "tanh" else (lambda v: v)
    xx = x.detach().clone().requires_grad_(True)
    t = xx[:, :, :3] + 1e-7
    r = torch.sqrt((t * t).sum(dim=2))
    live = r > 3e-6
    typ = torch.zeros_like(r) if lay.n_types == 1 else torch.round(xx[:, :, 3].detach())
    e = torch.exp(-(r[..., None] - mu) ** 2 / float(lay.gap))
    G = torch.cat([(e * (live & (typ == tt)).to(x.dtype)[..., None]).sum(dim=1) for tt in range(lay.n_types)], dim=1)
    h1 = act(G @ W[0] + W[1])
    h2 = act(h1 @ W[2] + W[3])
    E = (h2 @ W[4] + W[5])[:, 0]
    (g,) = torch.autograd.grad(E.sum(), xx, create_graph=True)
    return torch.cat([2.0 * g[:, :, :3].sum(dim=1), E[:, None]], dim=1)


def _weights64(lay, dev):
    return [torch.as_tensor(w.astype(np.float64), device=dev).requires_grad_(True) for w in lay.get_weights()]


def reference_gradient(lay, x, resid32, chunk=1024):
    """d SSR / d theta in fp64 by double backward, the residual being the sweep's own: (gradient [P], fp64 prediction [B, 4])."""
    W = _weights64(lay, x.device)
    total = [torch.zeros_like(w) for w in W]
    preds = []
    for s in range(0, x.shape[0], chunk):
        pred = net(lay, W, x[s:s + chunk].to(torch.float64))
        labels_eff = pred.detach() - resid32[s:s + chunk].to(torch.float64)
        ssr = ((pred - labels_eff) ** 2).sum()
        for acc, g in zip(total, torch.autograd.grad(ssr, W)):
            acc += g
        preds.append(pred.detach())
    return torch.cat([g.reshape(-1) for g in total]), torch.cat(preds)


def _blocks(lay):
    o = 0
    for k, shape in zip(_KEYS, lay._shapes):
        n = int(np.prod(shape))
        yield k, slice(o, o + n)
        o += n


def _check_gradient(lay, x, labels, accum, what):
    """accum against the fp64 reference fed the fp32 residual pred - labels; prints each figure before it asserts."""
    pred = lay.forces(x).to(torch.float32)
    resid = pred - labels.to(torch.float32)
    g, _ = reference_gradient(lay, x, resid)
    got = accum[1:].double()
    scale = g.abs().max().item()
    err = (got - g).abs().max().item()
    ssr = (resid.double() ** 2).sum().item()
    print("%s: max|got - g| = %.3g, max|g| = %.3g, ratio %.3g; SSR %.9g vs %.9g" % (what, err, scale, err / scale, accum[0].item(), ssr))
    for k, sl in _blocks(lay):
        print("   %s: max|g| = %.3g, max err = %.3g" % (k, g[sl].abs().max().item(), (got[sl] - g[sl]).abs().max().item()))
    assert np.isfinite(err) and scale > 0 and err < TOL * scale, "%s: max err %.3g of scale %.3g" % (what, err, scale)
    assert abs(accum[0].item() - ssr) <= 1e-5 * ssr, (accum[0].item(), ssr)
    for k, sl in _blocks(lay):
        assert g[sl].abs().max().item() > 0 and got[sl].abs().max().item() > 0, "%s carries no signal" % k
    return g


def _rows(cuda, n_types, NN, dtype, B=300, seed=0):
    """Random rows; row 0 has no live neighbor (padding with a nonzero column 3), row 1 out-of-range types beside good ones."""
    rng = np.random.default_rng(seed)
    nl, _ = random_nlist(rng, B, NN, fill=0.75, rmin=0.3, rmax=3.4, ntypes=n_types, dtype=np.float64)
    nl[0] = 0.0
    nl[0, :, 3] = 2.0
    nl[1, :8, 3] = [0, -1, n_types, 7, 2.6 if n_types == 3 else 0, 1 if n_types > 1 else 0, 0, -3]
    labels = 0.05 * rng.standard_normal((B, 4))
    return torch.from_numpy(nl).to(dtype).to(cuda), torch.from_numpy(labels).to(torch.float32).to(cuda)


# ------------------------------------------------------------------------------------------------ 1. the gradient
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("NN", [37, 128, 256])
@pytest.mark.parametrize("widths", ["ragged", "full"])
@pytest.mark.parametrize("n_types", [1, 3])
@pytest.mark.parametrize("activation", ["tanh", "linear"])
def test_gradient_against_fp64_double_backward(htf, cuda, activation, n_types, widths, NN, dtype):
    if widths == "ragged":
        K, H1, H2 = 16, 24, 20
    else:   # every lane a channel and a hidden unit (three types: 63 of the 64 channels)
        K, H1, H2 = 64 // n_types, 64, 64
    lay = _layer(htf, K=K, n_types=n_types, H1=H1, H2=H2, activation=activation, seed=5 + n_types)
    x, labels = _rows(cuda, n_types, NN, dtype, seed=7 + NN + 3 * n_types)
    accum = lay.loss_gradient(x, labels)
    assert accum.dtype == torch.float32 and accum.shape == (1 + lay.w.numel(),) and torch.isfinite(accum).all()
    _check_gradient(lay, x, labels, accum, "%s T=%d %s NN=%d %s" % (activation, n_types, widths, NN, dtype))
    # a prediction handed in is the one evaluated inside
    assert torch.equal(lay.loss_gradient(x, labels, pred=lay.forces(x).to(torch.float32)), accum)


# ------------------------------------------------------------------------------------------------ 2. reproducibility
def test_bitwise_reproducible_and_row_splits_add_up(htf, cuda):
    lay = _layer(htf, K=16, n_types=2, H1=64, H2=64)
    x, labels = _rows(cuda, 2, 128, torch.float32, B=999, seed=5)
    a = lay.loss_gradient(x, labels)
    b = lay.loss_gradient(x, labels)
    assert torch.equal(a, b)
    out = torch.full_like(a, float("nan"))
    assert lay.loss_gradient(x, labels, accum=out) is out and torch.equal(out, a)
    # three row splits: another order of the same sum, so the bound of (1) and not the same bits
    parts = sum(lay.loss_gradient(x[s:s + 333].contiguous(), labels[s:s + 333].contiguous()).double() for s in range(0, 999, 333))
    scale = a[1:].abs().max().item()
    err = (parts[1:] - a[1:].double()).abs().max().item()
    print("row splits: max diff %.3g of %.3g" % (err, scale))
    assert err < TOL * scale
    assert abs(parts[0].item() - a[0].item()) <= 1e-5 * a[0].item()


def test_zero_rows(htf, cuda):
    lay = _layer(htf, K=8, n_types=2)
    for dt in (torch.float32, torch.float64):
        acc = lay.loss_gradient(torch.zeros((0, 32, 4), dtype=dt, device=cuda), torch.zeros((0, 4), dtype=dt, device=cuda))
        assert acc.shape == (1 + lay.w.numel(),) and (acc == 0).all()


# ------------------------------------------------------------------------------------------------ 3. wire dtype
def test_fp64_tensors_give_the_fp32_call(htf, cuda):
    """fp64 labels and an fp64 pair-vector tensor holding the fp32 values: the bound the pair-MLP sweep's wire-dtype test uses."""
    lay = _layer(htf, K=16, n_types=3, H1=32, H2=48)
    x, labels = _rows(cuda, 3, 100, torch.float32, B=500, seed=11)
    a = lay.loss_gradient(x, labels).double()
    for xx, ll in ((x.double(), labels.double()), (x, labels.double()), (x.double(), labels)):
        b = lay.loss_gradient(xx, ll).double()
        err = (a - b).abs()
        print("wire dtype %s/%s: max diff %.3g of %.3g" % (xx.dtype, ll.dtype, err.max().item(), a.abs().max().item()))
        assert (err <= 1e-4 * a.abs() + 1e-5 * a.abs().max()).all()


# ------------------------------------------------------------------------------------------------ 4. full size
def test_gradient_full_size(htf, cuda):
    """N = 131 072, NN = 128, K = 32, 64 x 64, tanh, once: a 2 048-row block tiled 64 times, so that the reference is the
    block's fp64 gradient times 64 while every block of the grid and every partial of the reduction take part."""
    NN, nb, rep = 128, 2048, 64
    lay = _layer(htf, K=32, H1=64, H2=64, seed=9)
    xb, lb = _rows(cuda, 1, NN, torch.float32, B=nb, seed=31)
    x, labels = xb.repeat(rep, 1, 1).contiguous(), lb.repeat(rep, 1).contiguous()
    assert x.shape == (131072, NN, 4)
    accum = lay.loss_gradient(x, labels)
    pred_b = lay.forces(xb)
    assert torch.equal(lay.forces(x)[nb:2 * nb], pred_b)          # rows are batch independent: the block's residual is every tile's
    g, _ = reference_gradient(lay, xb, pred_b - lb)
    g, ssr = rep * g, rep * ((pred_b - lb).double() ** 2).sum().item()
    got = accum[1:].double()
    scale, err = g.abs().max().item(), (got - g).abs().max().item()
    print("full size: max|got - g| = %.3g, max|g| = %.3g, ratio %.3g; SSR %.9g vs %.9g" % (err, scale, err / scale, accum[0].item(), ssr))
    assert err < TOL * scale
    assert abs(accum[0].item() - ssr) <= 1e-5 * ssr


# ------------------------------------------------------------------------------------------------ 5. descent against torch twins
DESCENT_LR = 5e-4   # chosen on the CPU: the fp64 twin's loss falls at every one of the 30 steps (it still does at 1e-3, not at 3e-3)


def _descent_problem(htf, dev, trainable=True):
    """One fixed batch of 2 000 rows; the labels are the prediction of a teacher network of the same shape (other weights)."""
    B, NN = 2000, 64
    rng = np.random.default_rng(41)
    nl, _ = random_nlist(rng, B, NN, fill=0.7, rmin=0.7, rmax=2.9, dtype=np.float32)
    x = torch.from_numpy(nl).to(dev)
    kw = dict(K=16, H1=24, H2=20, low=0.5, high=3.0)
    lay = htf.DescriptorMLP(seed=4, trainable=trainable, device=dev, **kw)
    teacher = htf.DescriptorMLP(seed=17, device=dev, **kw)
    with torch.no_grad():
        W = [torch.as_tensor(w.astype(np.float64), device=dev) for w in teacher.get_weights()]
    labels = net(teacher, W, x.double()).detach().to(torch.float32)
    return lay, x, labels


def twin_descent(lay, x, labels, dtype, lr, steps):
    """Plain SGD theta <- theta - lr g / (4 B) on SSR, the network written in torch: (losses per step, final flat theta)."""
    W = [torch.as_tensor(w, device=x.device).to(dtype).requires_grad_(True) for w in lay.get_weights()]
    xx, ll = x.to(dtype), labels.to(dtype)
    B, losses = x.shape[0], []
    for _ in range(steps):
        ssr = ((net(lay, W, xx) - ll) ** 2).sum()
        gs = torch.autograd.grad(ssr, W)
        losses.append(ssr.item() / (4 * B))
        with torch.no_grad():
            for w, g in zip(W, gs):
                w -= lr * g / (4 * B)
    return losses, torch.cat([w.detach().reshape(-1) for w in W]).double()


def test_descent_tracks_torch_twins(htf, cuda):
    """30 SGD steps on fixed data through loss_gradient + ops.optimizer_step, beside the same network and rule in torch fp64
    and fp32.  The kernel path's weights may leave the fp64 twin's by at most 4x what the fp32 twin's do (the margin covers
    the different order of summation over rows and slots)."""
    from hoomd_tf_amd import ops
    steps = 30
    lay, x, labels = _descent_problem(htf, cuda)
    l64, t64 = twin_descent(lay, x, labels, torch.float64, DESCENT_LR, steps)
    l32, t32 = twin_descent(lay, x, labels, torch.float32, DESCENT_LR, steps)
    assert all(b < a for a, b in zip(l64, l64[1:])), l64
    state = torch.zeros(ops.optimizer_state_floats(lay.w.numel()), dtype=torch.float32, device=cuda)
    desc = htf.optimizers.SGD(DESCENT_LR).desc(lay.nonneg_mask, lay.l1_reg)
    B, losses = x.shape[0], []
    for _ in range(steps):
        accum = lay.loss_gradient(x, labels)
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


# ------------------------------------------------------------------------------------------------ 6. through tfcompute
def _fcc_sim(htf, cuda, seed):
    from hoomd_tf_amd import standin
    pos, L, a = standin.fcc_positions(5, 0.8442)
    rng = np.random.default_rng(seed)
    pos = pos + 0.03 * a * rng.standard_normal(pos.shape)
    pos -= np.round(pos / L) * L
    sysm = standin.System(pos, L, dtype=torch.float32, device=cuda)
    sysm.randomize_velocities(kT=0.3, seed=seed)
    sim = standin.Simulation(sysm)
    sim.integrate_nve(0.001)
    return sim, sysm


def _model(htf, lay):
    class M(htf.SimModel):
        def setup(self):
            self.desc = lay
            self.ops = []

        def compute(self, nlist, positions, box):
            log = htf.simmodel._trace_log()
            mark = len(log)
            out = htf.compute_nlist_forces(nlist, self.desc(nlist))
            self.ops.extend(e.get("op") for e in log[mark:])
            return out
    return M


def _training_run(htf, cuda, lay, optimizer, steps, batch_size=None, seed=23):
    """The set-up of test_gpu_desc.py::test_training_raises: an fcc box, LJModel driving the run and supplying the labels."""
    import build_examples
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


@pytest.mark.parametrize("batched", [False, True])
def test_training_through_tfcompute(htf, cuda, batched):
    lay = _layer(htf, K=8, H1=8, H2=8, high=2.5)
    w0 = lay.w.clone()
    model, tfc, sysm = _training_run(htf, cuda, lay, htf.optimizers.Adam(0.01), 30, batch_size=sysm_third() if batched else None)
    assert tfc._tplan is None and tfc._plan is None and tfc._train_seen is None
    nb = 3 if batched else 1
    assert "generic" not in model.ops and model.ops.count("descriptor_mlp") >= 30 * nb
    assert torch.isfinite(lay.w).all() and (lay.w - w0).abs().max().item() > 1e-3
    loss = float(model.metrics[0].result())
    print("tfcompute (%s): |dw| max %.3g, metric %.6g, last loss %.6g" % ("batches" if batched else "whole", (lay.w - w0).abs().max().item(),
                                                                         loss, float(tfc._opt_state[20])))
    assert np.isfinite(loss) and loss > 0


def sysm_third():
    return 500 // 3     # (the fcc box of _fcc_sim holds 4 * 5^3 = 500 particles)


def test_one_sgd_step_is_the_sweeps_gradient(htf, cuda):
    """After ONE SGD step from fresh weights, w - w0 = -lr g / (4 N), g from loss_gradient on the step's own tensor
    (get_nlist_array) and its staged labels.  The step is sized from a first, identical run so that max|dw| is about 0.25:
    fp32 weights of size ~0.5 are then stored to a few 1e-8, well inside the bound of 1e-6 max|dw|."""
    def run(lr):
        lay = _layer(htf, K=8, H1=8, H2=8, high=2.5)
        w0 = lay.w.clone()
        model, tfc, sysm = _training_run(htf, cuda, lay, htf.optimizers.SGD(lr), 1)
        x = torch.from_numpy(tfc.get_nlist_array()).to(torch.float32).to(cuda)
        fresh = _layer(htf, K=8, H1=8, H2=8, high=2.5)
        assert torch.equal(fresh.w, w0) and x.shape[0] == sysm.N
        g = fresh.loss_gradient(x, tfc._labels[:sysm.N].contiguous())[1:].double()
        return lay.w.double() - w0.double(), g, sysm.N

    _, g, N = run(1e-3)
    lr = 0.25 * 4 * N / g.abs().max().item()
    dw, g2, _ = run(lr)
    assert torch.equal(g2, g)
    want = -lr * g / (4 * N)
    err, scale = (dw - want).abs().max().item(), want.abs().max().item()
    print("one SGD step: lr %.4g, max|dw| %.3g, max err %.3g" % (lr, scale, err))
    assert err <= 1e-6 * scale


def test_default_layer_still_raises(htf, cuda):
    lay = _layer(htf, K=8, H1=8, H2=8, high=2.5, trainable=False)
    with pytest.raises(NotImplementedError, match="DescriptorMLP"):
        _training_run(htf, cuda, lay, htf.optimizers.Adam(0.01), 1)
