"""Force matching for every member of a committee in one sweep on the MI355X (csrc/cmt_train.hip, include/htf_cmt_train.h;
DescriptorMLP.committee_loss_gradient, trainable="committee"): per member, {SSR^m, d SSR^m / d theta^m} against

  (1) torch's fp64 double backward through the positions, tests/test_gpu_desc_total_train.reference_gradient on member m's
      weights, fed member m's own fp32 residual, with that module's bounds: 2e-4 of the largest gradient entry, the SSR to 1e-5;
  (2) member(m).total_loss_gradient, the single-network sweep, on the same residual: each side is within TOL of (1), so 2 TOL.

The systems are test_gpu_desc_total's jittered lattices; the committees are test_gpu_desc_committee's."""
import numpy as np
import pytest
import torch

import test_gpu_desc_total as T
import test_gpu_desc_total_train as TT
from test_gpu_desc_committee import _committee

pytestmark = pytest.mark.gpu
TOL = TT.TOL


def _layer(htf, M, **kw):
    """The committee of test_gpu_desc_committee at the widths of test_gpu_desc_total_train: 24 and 20 hidden units."""
    kw.setdefault("H1", 24)
    kw.setdefault("H2", 20)
    return _committee(htf, M, **kw)


def _residuals(pred, labels):
    """[M, B, 4] fp32, after the non-vacuity check: the members' residuals differ by at least 1e-2 of the largest, so a sweep
    that gathered another member's rho_j, or read another member's rho_i, is far outside every bound below."""
    rho = pred - labels.to(torch.float32)[None]
    spread = (rho - rho.mean(dim=0)).abs().max().item()
    assert spread >= 1e-2 * rho.abs().max().item(), "vacuous: the members' residuals agree"
    return rho


def _against_members(lay, x, labels, idx, accum, pred, what, species=None):
    """Reference (2): accum [M, 1 + P] (or [M, S, 1 + P]) against member(m).total_loss_gradient on pred[m]; the largest ratio."""
    worst = 0.0
    for m in range(lay.n_models):
        want = lay.member(m).total_loss_gradient(x, labels, idx, pred=pred[m].contiguous(), species=species)
        got = accum[m]
        assert got.shape == want.shape
        gg, ww = got.reshape(-1, 1 + lay.P).double(), want.reshape(-1, 1 + lay.P).double()
        for s in range(gg.shape[0]):
            scale = ww[s, 1:].abs().max().item()
            err = (gg[s, 1:] - ww[s, 1:]).abs().max().item()
            if scale == 0:
                assert err == 0 and gg[s, 0].item() == ww[s, 0].item() == 0, (what, m, s)
                continue
            worst = max(worst, err / scale)
            assert np.isfinite(err) and err < 2 * TOL * scale, "%s member %d: max err %.3g of scale %.3g" % (what, m, err, scale)
            assert abs(gg[s, 0].item() - ww[s, 0].item()) <= 1e-5 * ww[s, 0].item(), (what, m, s)
    print("%s: against member(m).total_loss_gradient, largest max err / max|g| = %.3g (bound %.3g)" % (what, worst, 2 * TOL))
    return worst


def _labels(B, cuda, seed):
    return torch.from_numpy(0.05 * np.random.default_rng(seed).standard_normal((B, 4))).to(torch.float32).to(cuda)


# ------------------------------------------------------------------------------------------------ 1. the gradient
# (M, system, n_types, cutoff, activation, dtype): K = 16 with one type, K = 10 with three; every value of every parameter at
# NN = 256 (b256) at least once
CASES = [
    (2, "a", 1, False, "tanh", torch.float32),
    (3, "a", 3, True, "linear", torch.float64),
    (8, "a", 1, True, "tanh", torch.float32),
    (2, "b", 3, False, "linear", torch.float32),
    (3, "b", 1, True, "tanh", torch.float64),
    (8, "b", 3, True, "tanh", torch.float32),
    (2, "b256", 1, True, "linear", torch.float64),
    (3, "b256", 3, False, "tanh", torch.float32),
    (8, "b256", 1, False, "tanh", torch.float64),
    (2, "b256", 3, True, "tanh", torch.float32),
    (3, "b256", 1, False, "linear", torch.float32),
    (8, "b256", 3, True, "linear", torch.float64),
]


@pytest.mark.parametrize("M,config,n_types,cut,activation,dtype", CASES)
def test_gradient_against_fp64_double_backward(htf, cuda, M, config, n_types, cut, activation, dtype):
    p, L, rc_list, x, idx = T._system(config)
    lay = _layer(htf, M, K=16 if n_types == 1 else 10, n_types=n_types, activation=activation, high=rc_list,
                 r_cut=0.9 * rc_list if cut else None, seed=5 + n_types)
    xx, types = x.to(dtype), p[:, 3].contiguous()
    labels = _labels(len(p), cuda, 7 + n_types)
    accum = lay.committee_loss_gradient(xx, labels, idx, types=types)
    assert accum.dtype == torch.float32 and accum.shape == (M, 1 + lay.P) and torch.isfinite(accum).all()
    pred = lay.total_forces(xx, idx, types=types, members=True)[-1]
    rho = _residuals(pred, labels)
    for m in range(M):
        g = TT.reference_gradient(lay.member(m), p, L, x, idx, rho[m])[0]
        TT._check(lay, accum[m, 1:], g, accum[m, 0].item(), (rho[m].double() ** 2).sum().item(),
                  "M=%d member %d %s T=%d %s cut=%s %s" % (M, m, config, n_types, activation, cut, dtype))


# ------------------------------------------------------------------------------------------------ 2. the single-network sweep
@pytest.mark.parametrize("M,config,n_types,dtype", [(2, "a", 3, torch.float64), (3, "b", 1, torch.float32), (8, "b256", 1, torch.float32)])
def test_against_the_single_network_sweep(htf, cuda, M, config, n_types, dtype):
    p, L, rc_list, x, idx = T._system(config)
    lay = _layer(htf, M, K=16 if n_types == 1 else 10, n_types=n_types, high=rc_list, r_cut=0.9 * rc_list, seed=21)
    xx, types = x.to(dtype), p[:, 3].contiguous()
    labels = _labels(len(p), cuda, 22)
    pred = lay.total_forces(xx, idx, types=types, members=True)[-1]
    _residuals(pred, labels)
    accum = lay.committee_loss_gradient(xx, labels, idx, types=types, pred=pred)
    assert _against_members(lay, xx, labels, idx, accum, pred, "M=%d %s" % (M, config)) < 2 * TOL


# ------------------------------------------------------------------------------------------------ 3. bits
def test_bits(htf, cuda):
    p, L, rc_list, x, idx = T._system("b")
    M = 3
    lay = _layer(htf, M, K=16, high=rc_list, r_cut=0.9 * rc_list, seed=31)
    labels = _labels(len(p), cuda, 32)
    a = lay.committee_loss_gradient(x, labels, idx)
    b = lay.committee_loss_gradient(x, labels, idx)
    assert torch.equal(a, b) and a[:, 1:].abs().amax(dim=1).min().item() > 0
    out = torch.full_like(a, float("nan"))
    assert lay.committee_loss_gradient(x, labels, idx, accum=out) is out and torch.equal(out, a)
    # a prediction handed in is the one evaluated inside; a float index is taken by rint
    pred = lay.total_forces(x, idx, members=True)[-1]
    assert torch.equal(lay.committee_loss_gradient(x, labels, idx, pred=pred), a)
    assert torch.equal(lay.committee_loss_gradient(x, labels, idx.to(torch.float32) + 0.25), a)
    # member 0's weights are nobody else's business
    with torch.no_grad():
        lay.w[:lay.P] *= 1.25
    c = lay.committee_loss_gradient(x, labels, idx)
    assert torch.equal(c[1:], a[1:]) and not torch.equal(c[0], a[0])
    # ... nor are its residuals: another prediction for member 0 alone
    pred2 = lay.total_forces(x, idx, members=True)[-1]
    pred2[0] += 0.125
    d = lay.committee_loss_gradient(x, labels, idx, pred=pred2)
    assert torch.equal(d[1:], a[1:]) and not torch.equal(d[0], c[0])


# ------------------------------------------------------------------------------------------------ 4. edges
def test_launch_above_64_kib_of_lds(htf, cuda):
    """M = 8 networks of 48 inputs and 32 x 24 units: 4 (8 (2468 + 640) + 16) = 99 520 bytes of dynamic LDS."""
    p, L, rc_list, x, idx = T._system("a")
    lay = _layer(htf, 8, K=16, n_types=3, H1=32, H2=24, high=rc_list, r_cut=0.9 * rc_list, seed=41)
    assert htf.DescriptorMLP.committee_train_lds_bytes(8, 16, 3, 32, 24) == 99520 > 64 * 1024
    labels, types = _labels(len(p), cuda, 42), p[:, 3].contiguous()
    pred = lay.total_forces(x, idx, types=types, members=True)[-1]
    _residuals(pred, labels)
    accum = lay.committee_loss_gradient(x, labels, idx, pred=pred)
    _against_members(lay, x, labels, idx, accum, pred, "M=8 D=48 32x24")


@pytest.mark.parametrize("NN", [1, 64, 65, 256])
def test_slots_per_lane(htf, cuda, NN):
    """The first NN slots of b256's rows (the list is no longer symmetric: reference (2) does not need it), H1 = 24, H2 = 20."""
    p, L, rc_list, x, idx = T._system("b256")
    x, idx = x[:, :NN].contiguous(), idx[:, :NN].contiguous()
    lay = _layer(htf, 3, K=10, n_types=3, high=rc_list, r_cut=0.9 * rc_list, seed=43)
    assert (lay.H1, lay.H2) == (24, 20)
    labels, types = _labels(len(p), cuda, 44), p[:, 3].contiguous()
    pred = lay.total_forces(x, idx, types=types, members=True)[-1]
    _residuals(pred, labels)
    accum = lay.committee_loss_gradient(x, labels, idx, pred=pred)
    _against_members(lay, x, labels, idx, accum, pred, "NN=%d" % NN)


def test_rows_and_indices_at_the_edges(htf, cuda):
    p, L, rc_list, x, idx = T._system("a")
    B = len(p)
    lay = _layer(htf, 2, K=16, high=rc_list, r_cut=0.9 * rc_list, seed=45)
    labels = _labels(B, cuda, 46)
    # a row with no live slot, and every third index of the others outside [0, B): no reverse term, nothing read there
    x2, idx2 = x.clone(), idx.clone()
    x2[5] = 0
    bad = torch.tensor([-1, B, 2 ** 31 - 1], dtype=torch.int32, device=cuda)
    flat = idx2.view(-1)
    flat[::3] = bad[torch.arange(flat[::3].numel(), device=cuda) % 3]
    pred = lay.total_forces(x2, idx2, members=True)[-1]
    _residuals(pred, labels)
    accum = lay.committee_loss_gradient(x2, labels, idx2, pred=pred)
    assert torch.isfinite(accum).all()
    _against_members(lay, x2, labels, idx2, accum, pred, "empty row, indices outside")
    full = lay.committee_loss_gradient(x2, labels, idx, pred=pred)
    assert (full[:, 1:] - accum[:, 1:]).abs().max().item() > 100 * TOL * accum[:, 1:].abs().max().item()   # (they were not small)
    # B = 1: every index is outside
    x1, idx1, l1 = x[:1].contiguous(), idx[:1].contiguous(), labels[:1].contiguous()
    pred1 = lay.total_forces(x1, idx1, members=True)[-1]
    acc1 = lay.committee_loss_gradient(x1, l1, idx1, pred=pred1)
    assert acc1.shape == (2, 1 + lay.P) and acc1[:, 1:].abs().amax(dim=1).min().item() > 0
    _against_members(lay, x1, l1, idx1, acc1, pred1, "B=1")
    # B = 0
    z = lay.committee_loss_gradient(torch.zeros((0, 32, 4), device=cuda), torch.zeros((0, 4), device=cuda),
                                    torch.zeros((0, 32), dtype=torch.int32, device=cuda))
    assert z.shape == (2, 1 + lay.P) and (z == 0).all()


def test_empty_row_list(htf, cuda):
    """n_rows = 0 with B > 0: the sweep is not launched and every member's [1 + P] is zero, whatever accum held; the stride
    between the members' results is the caller's."""
    from hoomd_tf_amd import ops
    L_ = htf._lib
    p, L, rc_list, x, idx = T._system("a")
    B, NN = x.shape[:2]
    lay = _layer(htf, 3, K=16, high=rc_list, seed=47)
    P, stride = lay.P, lay.P + 7
    rho = torch.ones((B, 3, 4), device=cuda)
    accum = torch.full((3, stride), float("nan"), device=cuda)
    rows = torch.zeros(1, dtype=torch.int32, device=cuda)
    assert int(L_.lib.htf_cmt_scratch_floats(0, lay.K, 1, lay.H1, lay.H2, 3)) == 0
    scratch = torch.empty(1, device=cuda)
    act = L_.ACT_TANH
    L_.check(L_.lib.htf_cmt_loss_grad(x.data_ptr(), ops._dt(x), idx.data_ptr(), B, NN, lay.K, 1, lay.H1, lay.H2, act, lay.w.data_ptr(),
                                      lay.mu.data_ptr(), float(lay.gap), rho.data_ptr(), accum.data_ptr(), scratch.data_ptr(),
                                      rows.data_ptr(), 0, 0.0, 3, P, stride, ops._stream(x)))
    assert (accum[:, :1 + P] == 0).all() and torch.isnan(accum[:, 1 + P:]).all()


# ------------------------------------------------------------------------------------------------ 5. species
def test_one_network_per_species(htf, cuda):
    p, L, rc_list, x, idx = T._system("a")
    B, M = len(p), 3
    lay = _layer(htf, M, K=10, n_types=3, high=rc_list, r_cut=0.9 * rc_list, n_species=2, seed=51)
    types, labels = p[:, 3].contiguous(), _labels(B, cuda, 52)
    # every particle in species 1: network 0 of every member has no rows
    ones = torch.ones(B, device=cuda)
    pred = lay.total_forces(x, idx, types=types, species=ones, members=True)[-1]
    _residuals(pred, labels)
    accum = lay.committee_loss_gradient(x, labels, idx, types=types, species=ones, accum=torch.full((M, 2, 1 + lay.P), float("nan"),
                                                                                                      device=cuda))
    assert accum.shape == (M, 2, 1 + lay.P) and (accum[:, 0] == 0).all() and accum[:, 1, 1:].abs().amax(dim=1).min().item() > 0
    _against_members(lay, x, labels, idx, accum, pred, "one species absent", species=ones)
    rho = pred - labels[None]
    for m in range(M):
        g = TT.reference_gradient(lay.member(m), p, L, x, idx, rho[m], sp=ones.long())
        assert (g[0] == 0).all()
        TT._check(lay, accum[m, 1, 1:], g[1], accum[m, 1, 0].item(), (rho[m].double() ** 2).sum().item(), "species 1, member %d" % m)
    # both present
    sp = torch.from_numpy(np.random.default_rng(53).integers(0, 2, B)).to(cuda).to(torch.float32)
    pred = lay.total_forces(x, idx, types=types, species=sp, members=True)[-1]
    both = lay.committee_loss_gradient(x, labels, idx, types=types, species=sp)
    assert both[:, :, 1:].abs().amax(dim=2).min().item() > 0
    _against_members(lay, x, labels, idx, both, pred, "two species", species=sp)


# ------------------------------------------------------------------------------------------------ 6. in the run
def _tf_committee(htf, trainable):
    """fc vanishes before the list's cutoff 2.5: the step's list is symmetric within the descriptor's range."""
    return htf.DescriptorMLP(K=8, H1=8, H2=8, low=0.5, high=2.5, r_cut=2.0, n_models=2, conservative=True, trainable=trainable)


def _attach(htf, sim_nlist, lj, lay, lr):
    model = TT._model(htf, lay)(128, output_forces=False)
    model.compile(htf.optimizers.SGD(lr), loss='MeanSquaredError')
    tfc = htf.tfcompute(model)
    tfc.attach(sim_nlist, train=True, r_cut=2.5)
    tfc.set_reference_forces(lj)
    return model, tfc


def test_training_through_tfcompute(htf, cuda):
    """Three SGD steps of tfcompute(train=True) on a committee of two beside two single trainable="total" layers started from
    the members' weights and trained in the same run (LJ drives and labels; nothing trained acts on the particles): member m's
    weights are the single layer's to 1e-5 of max|w|, and the reported loss is the mean of the two."""
    import build_examples
    from test_gpu_desc_train import _fcc_sim
    steps, lr = 3, 0.05
    sim, sysm = _fcc_sim(htf, cuda, seed=29)
    nlist = sim.nlist_cell()
    lj = htf.tfcompute(build_examples.LJModel(128))
    lj.attach(nlist, r_cut=2.5)
    lay = _tf_committee(htf, "committee")
    assert lay.trainable == "committee" and lay.conservative and lay.n_models == 2
    w0, P = lay.w.clone(), lay.P
    singles = []
    for m in range(2):
        one = htf.DescriptorMLP(K=8, H1=8, H2=8, low=0.5, high=2.5, r_cut=2.0, trainable="total")
        with torch.no_grad():
            one.w.copy_(w0[m * P:(m + 1) * P])
        singles.append((one,) + _attach(htf, nlist, lj, one, lr))
    model, tfc = _attach(htf, nlist, lj, lay, lr)
    sim.run(steps)
    torch.cuda.synchronize()
    assert tfc._tplan is None and tfc._plan is None and tfc._train_seen is None   # (eager: no train plan)
    assert "generic" not in model.ops and model.ops.count("descriptor_mlp") >= steps
    assert torch.isfinite(lay.w).all()
    losses = []
    for m, (one, model1, tfc1) in enumerate(singles):
        got, want = lay.w[m * P:(m + 1) * P].double(), one.w.double()
        moved = (want - w0[m * P:(m + 1) * P].double()).abs().max().item()
        err, scale = (got - want).abs().max().item(), want.abs().max().item()
        print("in the run, member %d: max|w - w_single| = %.3g of max|w| = %.3g, ratio %.3g (moved by %.3g)"
              % (m, err, scale, err / scale, moved))
        assert moved > 1e-3 * scale, "vacuous: the single layer did not train"
        assert err <= 1e-5 * scale
        losses.append((float(tfc1._opt_state[20]), float(model1.metrics[0].result())))
    last, metric = float(tfc._opt_state[20]), float(model.metrics[0].result())
    print("in the run: last loss %.9g, members' %.9g and %.9g; metric %.9g, members' %.9g and %.9g"
          % (last, losses[0][0], losses[1][0], metric, losses[0][1], losses[1][1]))
    assert abs(losses[0][0] - losses[1][0]) > 1e-3 * last, "vacuous: the members' losses agree"
    assert abs(last - 0.5 * (losses[0][0] + losses[1][0])) <= 1e-5 * last
    assert abs(metric - 0.5 * (losses[0][1] + losses[1][1])) <= 1e-5 * metric


def test_a_committee_that_is_not_trainable_still_raises(htf, cuda):
    import build_examples
    from test_gpu_desc_train import _fcc_sim
    sim, sysm = _fcc_sim(htf, cuda, seed=29)
    nlist = sim.nlist_cell()
    lj = htf.tfcompute(build_examples.LJModel(128))
    lj.attach(nlist, r_cut=2.5)
    _attach(htf, nlist, lj, _tf_committee(htf, False), 1e-3)
    with pytest.raises(NotImplementedError, match="member"):
        sim.run(1)
