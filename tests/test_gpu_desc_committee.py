"""htf.DescriptorMLP(conservative=True, n_models=M) on the MI355X (csrc/committee.hip, include/htf_committee.h): the mean-model
conservative forces and the per-particle deviation of a committee of M networks,

    Ebar_i = (1/M) sum_m E_i^m        Fbar_i = (1/M) sum_m F_i^m        Wbar_i = (1/M) sum_m W_i^m
    devF_i = sqrt((1/M) sum_m |F_i^m - Fbar_i|^2)        devE_i = sqrt((1/M) sum_m (E_i^m - Ebar_i)^2)

against the references of test_gpu_desc_total.py evaluated once per member: the fp64 autograd oracle of the definition, and the
fp64 formula of include/htf_cforce.h for virials and dropped reverse terms.  Systems, shapes and the bias trick are that file's.

Bounds.  Means: TOL = 2e-5 of the largest reference magnitude, the project's bound for this arithmetic.  Deviations:
2 TOL max_{m,i} |F_i^m| (likewise with energies), absolute: the deviation is an RMS, a 1-Lipschitz function, of the members'
errors taken relative to their mean, and each of the two carries at most TOL.  Every reference-based case first asserts that it
is not vacuous: max_i devF_i >= 1e-2 max |F_i^m| on the reference."""
import numpy as np
import pytest
import torch

from test_gpu_desc_total import TOL, _close, _descriptor, _model, _network, _sim, _system, formula, oracle

pytestmark = pytest.mark.gpu


def _committee(htf, M, K=16, n_types=1, activation="tanh", high=1.8, r_cut=None, n_species=1, seed=3, H1=32, H2=24, bias=0.1):
    """test_gpu_desc_total._layer with n_models=M: mlp_params' zero biases replaced, or the bias paths would stay untested."""
    lay = htf.DescriptorMLP(K=K, H1=H1, H2=H2, low=0.5, high=high, n_types=n_types, activation=activation, seed=seed,
                            r_cut=r_cut, n_species=n_species, conservative=True, n_models=M)
    rng = np.random.default_rng(seed + 100)
    ws = lay.get_weights()
    for i in (1, 3, 5):
        ws[i] = (bias * rng.standard_normal(ws[i].shape)).astype(np.float32)
    lay.set_weights(ws)
    return lay


def _stats(Fm, Em):
    """(Fbar, Ebar, devF, devE) of members' forces [M, B, 3] and energies [M, B] in fp64, after the non-vacuity check."""
    Fbar, Ebar = Fm.mean(dim=0), Em.mean(dim=0)
    devF = ((Fm - Fbar) ** 2).sum(dim=2).mean(dim=0).sqrt()
    devE = ((Em - Ebar) ** 2).mean(dim=0).sqrt()
    assert devF.max().item() >= 1e-2 * Fm.abs().max().item(), "vacuous: the members agree"
    return Fbar, Ebar, devF, devE


def _check_against(f, dev, Fm, Em):
    Fbar, Ebar, devF, devE = _stats(Fm, Em)
    _close(f[:, :3], Fbar, "mean forces", scale=Fm.abs().max().item())
    _close(f[:, 3], Ebar, "mean energy", scale=Em.abs().max().item())
    _close(dev[:, 0], devF, "devF", tol=2 * TOL, scale=Fm.abs().max().item())
    _close(dev[:, 1], devE, "devE", tol=2 * TOL, scale=Em.abs().max().item())


def _oracle_members(lay, p, L, x, idx, sp=None):
    ref = [oracle(lay.member(m), p, L, x, idx, sp=sp) for m in range(lay.n_models)]
    return torch.stack([r[0] for r in ref]), torch.stack([r[1] for r in ref])


def _formula_members(lay, x, idx, ti):
    ref = [formula(lay.member(m), x, idx, ti) for m in range(lay.n_models)]
    return torch.stack([r[0] for r in ref]), torch.stack([r[1] for r in ref]), torch.stack([r[2] for r in ref])


# ------------------------------------------------------------------------------------------------ 1. values
# (M, shape, K, n_types, cutoff, activation, dtype): every value of every parameter at NN = 256 (b256) at least once; K = 6 is
# the gather by single floats, K = 16 by float4; M = 8 with 48 inputs is the launch above 64 KiB of LDS
CASES = [
    (2, "b256", 16, 1, False, "tanh", torch.float32),
    (3, "b256", 6, 3, True, "linear", torch.float64),
    (8, "b256", 16, 3, True, "tanh", torch.float32),
    (8, "b256", 6, 1, False, "linear", torch.float64),
    (3, "b256", 16, 1, True, "tanh", torch.float64),
    (2, "b256", 6, 3, False, "tanh", torch.float32),
    (2, "a", 16, 1, True, "tanh", torch.float32),
    (2, "a", 6, 3, False, "linear", torch.float64),
    (2, "a", 16, 3, True, "linear", torch.float32),
    (3, "a", 16, 3, False, "tanh", torch.float64),
    (3, "a", 6, 1, True, "tanh", torch.float32),
    (3, "a", 16, 1, False, "linear", torch.float32),
    (8, "a", 16, 1, True, "linear", torch.float64),
    (8, "a", 6, 3, True, "tanh", torch.float32),
    (8, "a", 16, 3, False, "tanh", torch.float64),
    (2, "b", 16, 3, False, "tanh", torch.float64),
    (2, "b", 6, 1, True, "linear", torch.float32),
    (2, "b", 16, 1, False, "linear", torch.float64),
    (3, "b", 16, 1, True, "linear", torch.float32),
    (3, "b", 6, 3, False, "tanh", torch.float32),
    (3, "b", 16, 3, True, "tanh", torch.float64),
    (8, "b", 16, 3, True, "linear", torch.float32),
    (8, "b", 6, 1, False, "tanh", torch.float64),
    (8, "b", 16, 1, True, "tanh", torch.float32),
]


@pytest.mark.parametrize("M,config,K,n_types,cut,activation,dtype", CASES)
def test_means_and_deviation(htf, cuda, M, config, K, n_types, cut, activation, dtype):
    p, L, rc_list, x, idx = _system(config)
    lay = _committee(htf, M, K=K, n_types=n_types, activation=activation, high=rc_list, r_cut=0.9 * rc_list if cut else None,
                     seed=5 + n_types)
    assert lay.deviation is None
    nl = htf.Nlist(x.to(dtype), index=idx)
    f = htf.compute_nlist_forces(nl, lay(nl, p.to(dtype)))
    dev = lay.deviation
    assert f.dtype == dtype and f.shape == (len(p), 4)
    assert dev.dtype == torch.float32 and dev.shape == (len(p), 2)
    _check_against(f, dev, *_oracle_members(lay, p, L, x, idx))


# ------------------------------------------------------------------------------------------------ 2. the members
@pytest.mark.parametrize("M,config,K,n_types", [(3, "a", 16, 3), (8, "b256", 16, 1), (2, "b256", 6, 3)])
def test_members(htf, cuda, M, config, K, n_types):
    """Block m of the members is the single-network kernels' total_forces of member(m) within TOL, and the mean returned is
    within 2^-22 max_m |x^m| of the exact mean of the fp32 members: the pairwise sum of at most 8 values rounds three times
    and the division once, each by at most 2^-24 of a partial sum no larger than M max_m |x^m|."""
    p, L, rc_list, x, idx = _system(config)
    types = p[:, 3].contiguous()
    lay = _committee(htf, M, K=K, n_types=n_types, high=rc_list, r_cut=0.9 * rc_list, seed=13)
    f, mem = lay.total_forces(x, idx, types=types, members=True)
    assert mem.shape == (M, len(p), 4) and mem.dtype == torch.float32
    fv, v, mem2 = lay.total_forces(x, idx, virial=True, types=types, members=True)
    assert torch.equal(fv, f) and torch.equal(mem2, mem) and v.shape == (len(p), 3, 3)
    for m in range(M):
        one = lay.member(m).total_forces(x, idx, types=types)
        _close(mem[m, :, :3], one[:, :3], "member %d forces" % m)
        _close(mem[m, :, 3], one[:, 3], "member %d energy" % m)
    exact = mem.double().mean(dim=0)
    bound = 2.0 ** -22 * mem.double().abs().max(dim=0).values
    assert bool(((f.double() - exact).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------ 3. identical members
@pytest.mark.parametrize("M", [2, 8])
def test_identical_members(htf, cuda, M):
    """Every member given the same weights: the two-pass deviation leaves a few ulps (about 1e-7) at most, the cancelling form
    <x^2> - <x>^2 about sqrt(2^-24) = 2.4e-4; 1e-6 separates them."""
    p, L, rc_list, x, idx = _system("b")
    one = _committee(htf, 2, K=16, n_types=3, high=rc_list, r_cut=0.9 * rc_list, seed=17).member(1)
    lay = _committee(htf, M, K=16, n_types=3, high=rc_list, r_cut=0.9 * rc_list, seed=19)
    lay.set_weights([np.broadcast_to(w, (M,) + w.shape).copy() for w in one.get_weights()])
    types = p[:, 3].contiguous()
    f = lay.total_forces(x, idx, types=types)
    ref = one.total_forces(x, idx, types=types)
    assert ref[:, :3].abs().max().item() > 1e-3
    assert lay.deviation[:, 0].max().item() <= 1e-6 * ref[:, :3].abs().max().item()
    assert lay.deviation[:, 1].max().item() <= 1e-6 * ref[:, 3].abs().max().item()
    _close(f[:, :3], ref[:, :3], "mean forces")
    _close(f[:, 3], ref[:, 3], "mean energy")


# ------------------------------------------------------------------------------------------------ 4. one network per species
def test_one_network_per_species(htf, cuda):
    """n_species = 2, n_models = 2 over a system of three types with n_types = 2 (test_gpu_desc_total's case), then the same
    layer on a batch in which species 1 is absent."""
    p, L, rc_list, x, idx = _system("a")
    lay = _committee(htf, 2, K=20, n_types=2, high=rc_list, r_cut=0.9 * rc_list, n_species=2, seed=11)
    assert lay.w.numel() == 2 * 2 * lay.P
    types = p[:, 3].contiguous()
    for sp in (p[:, 3].long() % 2, torch.zeros(len(p), dtype=torch.long, device=cuda)):
        f = lay.total_forces(x, idx, types=types, species=sp.to(torch.float32))
        _check_against(f, lay.deviation, *_oracle_members(lay, p, L, x, idx, sp=sp))


# ------------------------------------------------------------------------------------------------ 5. the mean virial
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("config", ["a", "b256"])
def test_mean_virial(htf, cuda, config, cut, dtype):
    p, L, rc_list, x, idx = _system(config)
    lay = _committee(htf, 3, K=16, n_types=3, high=rc_list, r_cut=0.9 * rc_list if cut else None, seed=31)
    xx = x.to(dtype)
    nl = htf.Nlist(xx, index=idx)
    f, w = htf.compute_nlist_forces(nl, lay(nl, p.to(dtype)), virial=True)
    assert w.dtype == dtype and w.shape == (len(p), 3, 3)
    Fm, Em, Wm = _formula_members(lay, x, idx, p[:, 3].long())
    _check_against(f, lay.deviation, Fm, Em)
    _close(w, Wm.mean(dim=0), "mean virial", scale=Wm.abs().max().item())
    # without the virial: the same forces and deviation, bit for bit
    dev = lay.deviation
    assert torch.equal(htf.compute_nlist_forces(nl, lay(nl, p.to(dtype))), f) and torch.equal(lay.deviation, dev)


# ------------------------------------------------------------------------------------------------ 6. edges
def test_edges(htf, cuda):
    """test_gpu_desc_total.test_edges for every member: indices outside [0, B) on live slots drop that slot's reverse term and
    nothing else; a row whose own type is out of range gathers nothing; a row of empty slots has no force, no force deviation
    and the energies of G = 0."""
    p, L, rc_list, x, idx = _system("a")
    B, M = len(p), 3
    lay = _committee(htf, M, K=16, n_types=3, high=rc_list, seed=51)
    x, idx, types = x.clone(), idx.clone(), p[:, 3].clone()
    idx[0, 0], idx[1, 0], idx[2, 1], idx[3, 2] = -1, B, B + 5, -7
    x[5] = 0.0
    types[7] = 3.0
    f, w, mem = lay.total_forces(x, idx, virial=True, types=types, members=True)
    dev = lay.deviation
    assert torch.isfinite(f).all() and torch.isfinite(w).all() and torch.isfinite(dev).all() and torch.isfinite(mem).all()
    Fm, Em, Wm = _formula_members(lay, x, idx, types.long())
    _check_against(f, dev, Fm, Em)
    _close(w, Wm.mean(dim=0), "mean virial", scale=Wm.abs().max().item())
    for m in range(M):
        _close(mem[m, :, :3], Fm[m], "member %d forces" % m)
    # the dropped terms are not small, in any member
    for m in range(M):
        Fall = formula(lay.member(m), x, _system("a")[4], types.long())[0]
        assert (Fall[:4] - Fm[m, :4]).abs().max().item() > 100 * TOL * Fm[m].abs().max().item()
    assert (f[5, :3] == 0).all() and (w[5] == 0).all() and (mem[:, 5, :3] == 0).all() and dev[5, 0].item() == 0
    for m in range(M):
        e0 = _network(lay.member(m), torch.zeros((1, lay.D), dtype=torch.float64, device=cuda),
                      torch.zeros(1, dtype=torch.long, device=cuda))
        assert abs(mem[m, 5, 3].item() - e0.item()) <= 1e-6 * max(1.0, abs(e0.item()))


def test_zero_rows(htf, cuda):
    lay = _committee(htf, 2, K=8, n_types=2)
    for dt in (torch.float32, torch.float64):
        x = torch.zeros((0, 32, 4), dtype=dt, device=cuda)
        f, v, mem = lay.total_forces(x, torch.zeros((0, 32), dtype=torch.int32, device=cuda), virial=True,
                                     types=torch.zeros((0,), device=cuda), members=True)
        assert f.shape == (0, 4) and v.shape == (0, 3, 3) and f.dtype == dt
        assert mem.shape == (2, 0, 4) and lay.deviation.shape == (0, 2)


# ------------------------------------------------------------------------------------------------ 7. bits
def test_bits(htf, cuda):
    p, L, rc_list, x, idx = _system("a")
    lay = _committee(htf, 3, K=6, n_types=3, high=rc_list, r_cut=0.9 * rc_list, seed=41)
    types = p[:, 3].contiguous()
    a = lay.total_forces(x, idx, virial=True, types=types, members=True)
    da = lay.deviation
    b = lay.total_forces(x, idx, virial=True, types=types, members=True)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.equal(da, lay.deviation)
    # the rows in another order, the index remapped: the same bits per particle
    perm = torch.randperm(len(p), generator=torch.Generator().manual_seed(7)).to(cuda)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(len(p), device=cuda)
    idx2 = torch.where(idx >= 0, inv[idx.clamp(min=0).long()].to(torch.int32), idx)[perm].contiguous()
    c = lay.total_forces(x[perm].contiguous(), idx2, virial=True, types=types[perm].contiguous(), members=True)
    assert a[0][:, :3].abs().max().item() > 0
    assert torch.equal(c[0], a[0][perm]) and torch.equal(c[1], a[1][perm]) and torch.equal(c[2], a[2][:, perm])
    assert torch.equal(lay.deviation, da[perm])


# ------------------------------------------------------------------------------------------------ 8. through tfcompute
def test_nve_through_tfcompute(htf, cuda):
    """test_gpu_desc_total.test_nve_through_tfcompute with a committee of 3: five NVE steps of 500 particles, r_cut = 2.0 under
    a list cutoff 2.5.  The last forces are the mean over the members of the all-pairs fp64 gradient, and a model that returns
    (forces, layer.deviation) leaves the deviation in tfcompute.outputs."""
    lay = _committee(htf, 3, K=16, high=2.0, r_cut=2.0, seed=71)
    sim, sysm, L = _sim(htf, cuda, 73)

    class M(htf.SimModel):
        def setup(self):
            self.desc = lay
            self.seen = None

        def compute(self, nlist, positions, box):
            self.seen = positions.detach().clone()
            f = htf.compute_nlist_forces(nlist, self.desc(nlist, positions))
            return f, self.desc.deviation

    model = M(128)
    tfc = htf.tfcompute(model)
    tfc.attach(sim.nlist_cell(), r_cut=2.5, save_output_period=1)
    sim.run(5)
    torch.cuda.synchronize()
    assert tfc._plan is None
    f = sysm.force[:sysm.N].double()
    Fm, Em = [], []
    for m in range(3):
        q = model.seen[:, :3].double().requires_grad_(True)
        d = q[None, :, :] - q[:, None, :]
        d = d - L * torch.round(d.detach() / L)
        off = ~torch.eye(sysm.N, dtype=torch.bool, device=cuda)
        one = lay.member(m)
        G = _descriptor(one, d * off[..., None].to(d.dtype), torch.zeros((sysm.N, sysm.N), dtype=torch.float64, device=cuda))[0]
        E = _network(one, G, torch.zeros(sysm.N, dtype=torch.long, device=cuda))
        (g,) = torch.autograd.grad(E.sum(), q)
        Fm.append(-g)
        Em.append(E.detach())
    _check_against(f, lay.deviation, torch.stack(Fm), torch.stack(Em))
    assert len(tfc.outputs) == 1 and tfc.outputs[0].shape[1:] == (sysm.N, 2)
    assert np.array_equal(tfc.outputs[0][-1], lay.deviation.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 9. what raises
def test_raises(htf, cuda):
    kw = dict(K=8, H1=8, H2=8, conservative=True)
    for bad in (0, 9, -1, 2.0, "2", True, None):
        with pytest.raises(ValueError, match="n_models.*total_forces"):
            htf.DescriptorMLP(n_models=bad, **kw)
    with pytest.raises(ValueError, match="conservative=True.*total_forces"):
        htf.DescriptorMLP(K=8, H1=8, H2=8, n_models=2)
    with pytest.raises(NotImplementedError, match="l_max.*follow-up.*total_forces"):
        htf.DescriptorMLP(l_max=1, n_models=2, **kw)
    for tr in (True, "total"):
        with pytest.raises(NotImplementedError, match="trainable.*follow-up.*member"):
            htf.DescriptorMLP(trainable=tr, n_models=2, **kw)
    # over the LDS budget: 8 x 34 KB, at construction, both byte counts in the message
    need = htf.DescriptorMLP.committee_lds_bytes(8, 64, 1, 64, 64)
    assert need > 8 * 34000
    with pytest.raises(ValueError, match=r"%d bytes.*%d bytes" % (need, 160 * 1024)):
        htf.DescriptorMLP(K=64, H1=64, H2=64, conservative=True, n_models=8)
    p, L, rc_list, x, idx = _system("a")
    lay = _committee(htf, 2, K=8, high=rc_list)
    with pytest.raises(NotImplementedError, match="follow-up.*member"):
        lay.total_forces(x, idx, n_ghost=4, halo=lambda t: None)
    labels = torch.zeros((len(p), 4), device=cuda)
    for what, call in (("forces", lambda: lay.forces(x)), ("loss_gradient", lambda: lay.loss_gradient(x, labels)),
                       ("total_loss_gradient", lambda: lay.total_loss_gradient(x, labels, idx)),
                       ("angular_loss_gradient", lambda: lay.angular_loss_gradient(x, labels, idx)),
                       ("descriptor", lambda: lay.descriptor(htf.Nlist(x)))):
        with pytest.raises(NotImplementedError, match=r"member\(m\)\.%s" % what):
            call()
    with pytest.raises(ValueError, match="committee"):
        lay.member(0).total_forces(x, idx, members=True)
    with pytest.raises(ValueError, match="member"):
        lay.member(2)
    # a committee under tfcompute(train=True)
    # (the run of test_gpu_desc_total_train: LJ drives and labels)
    import build_examples
    sim, sysm, _ = _sim(htf, cuda, 83)
    nlist = sim.nlist_cell()
    lj = htf.tfcompute(build_examples.LJModel(128))
    lj.attach(nlist, r_cut=2.5)
    model = _model(htf, _committee(htf, 2, K=8, high=2.0, r_cut=2.0))(128, output_forces=False)
    model.compile(htf.optimizers.SGD(1e-3), loss='MeanSquaredError')
    tfc = htf.tfcompute(model)
    tfc.attach(nlist, train=True, r_cut=2.5)
    tfc.set_reference_forces(lj)
    with pytest.raises(NotImplementedError, match="member"):
        sim.run(1)


# ------------------------------------------------------------------------------------------------ 10. training through the view
def test_training_through_member_view(htf, cuda):
    """One total_loss_gradient and one optimizer step on member(1, trainable="total") change member 1's slice of the committee's
    w and no other, and the committee's next call shows it: block 1 of the members moves, blocks 0 and 2 keep their bits."""
    from hoomd_tf_amd import ops
    p, L, rc_list, x, idx = _system("a")
    lay = _committee(htf, 3, K=16, high=rc_list, r_cut=0.9 * rc_list, seed=61)
    n = lay.n_species * lay.P
    before_w = lay.w.clone()
    _, before = lay.total_forces(x, idx, members=True)
    one = lay.member(1, trainable="total")
    assert one.trainable == "total" and one.n_models == 1 and one.w.data_ptr() == lay.w.data_ptr() + 4 * n
    labels = torch.zeros((len(p), 4), device=cuda)
    accum = one.total_loss_gradient(x, labels, idx)
    state = torch.zeros(ops.optimizer_state_floats(one.w.numel()), dtype=torch.float32, device=cuda)
    ops.optimizer_step(one.w, accum, 1.0 / (4 * len(p)), state, htf.optimizers.SGD(1e-2).desc(one.nonneg_mask, one.l1_reg))
    torch.cuda.synchronize()
    assert torch.equal(lay.w[:n], before_w[:n]) and torch.equal(lay.w[2 * n:], before_w[2 * n:])
    assert not torch.equal(lay.w[n:2 * n], before_w[n:2 * n])
    _, after = lay.total_forces(x, idx, members=True)
    assert torch.equal(after[0], before[0]) and torch.equal(after[2], before[2])
    assert (after[1] - before[1]).abs().max().item() > 0
