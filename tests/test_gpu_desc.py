"""htf.DescriptorMLP on the MI355X (csrc/bp.hip over desc_row.h) against an fp64 torch-autograd restatement of its definition:

    r_ij = sqrt(sum_c (x_ij,c + 1e-7)^2), live_ij = r_ij > 3e-6, t_ij = 0 (n_types = 1) or rint(nlist[i, j, 3])
    G_i[t*K + k] = sum_j live_ij [t_ij = t] exp(-(r_ij - mu_k)^2 / gap)
    E_i = W3^T act(W2^T act(W1^T G_i + b1) + b2) + b3,  f_i = 2 sum_j dE_i/dx_ij,  virial: the generic route's formula.

Bounds are 2e-5 of the largest reference value, as the descriptor test of the generic route uses (fp32 arithmetic over at
most 256 slots and 64-wide layers)."""
import numpy as np
import pytest
import torch

from helpers import random_nlist

pytestmark = pytest.mark.gpu
TOL = 2e-5


def _layer(htf, K=16, n_types=1, H1=32, H2=32, activation="tanh", low=0.0, high=3.0, seed=3, bias=0.1):
    lay = htf.DescriptorMLP(K=K, H1=H1, H2=H2, low=low, high=high, n_types=n_types, activation=activation, seed=seed)
    if bias:   # (mlp_params' zero biases would leave the bias paths untested)
        rng = np.random.default_rng(seed + 100)
        ws = lay.get_weights()
        for i in (1, 3, 5):
            ws[i] = (bias * rng.standard_normal(ws[i].shape)).astype(np.float32)
        lay.set_weights(ws)
    return lay


def reference(lay, x, virial=True, chunk=8192):
    """fp64 autograd of the definition, on x's device, in row chunks: (F [B, 3], E [B], G [B, D], V [B, 3, 3])."""
    dev = x.device
    mu = torch.as_tensor(lay.centers.astype(np.float64), device=dev)
    gap = float(lay.gap)
    W = [torch.as_tensor(w.astype(np.float64), device=dev) for w in lay.get_weights()]
    act = torch.tanh if lay.activation == "tanh" else (lambda v: v)
    outs = [[], [], [], []]
    for s in range(0, max(x.shape[0], 1), chunk):
        xx = x[s:s + chunk].detach().to(torch.float64).clone().requires_grad_(True)
        t = xx[:, :, :3] + 1e-7
        r = torch.sqrt((t * t).sum(dim=2))
        live = r > 3e-6
        typ = torch.zeros_like(r) if lay.n_types == 1 else torch.round(xx[:, :, 3].detach())
        e = torch.exp(-(r[..., None] - mu) ** 2 / gap)
        G = torch.cat([(e * (live & (typ == tt)).to(torch.float64)[..., None]).sum(dim=1) for tt in range(lay.n_types)], dim=1)
        h1 = act(G @ W[0] + W[1])
        h2 = act(h1 @ W[2] + W[3])
        E = (h2 @ W[4] + W[5])[:, 0]
        (g,) = torch.autograd.grad(E.sum(), xx, allow_unused=True)
        g = torch.zeros_like(xx) if g is None else g
        nf = 2.0 * g[:, :, :3]
        outs[0].append(nf.sum(dim=1))
        outs[1].append(E.detach())
        outs[2].append(G.detach())
        if virial:
            n3 = xx[:, :, :3].detach()
            rmag = torch.sqrt((n3 * n3).sum(dim=2))
            fmag = torch.sqrt((nf * nf).sum(dim=2))
            den = 2.0 * rmag
            frs = torch.where(den == 0, torch.zeros_like(den), fmag / den)
            outs[3].append(-1.0 * torch.einsum("ij,ijk,ijl->ikl", frs, n3, n3))
        if x.shape[0] == 0:
            break
    return tuple(torch.cat(o) if o else None for o in outs)


def _close(got, ref, what, tol=TOL):
    got, ref = got.double(), ref.double()
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    assert np.isfinite(err) and err <= tol * scale, "%s: max err %.3g of scale %.3g" % (what, err, scale)


def _forces(htf, lay, x, virial=True):
    nl = htf.Nlist(x)
    return htf.compute_nlist_forces(nl, lay(nl), virial=virial)


# ------------------------------------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("NN", [37, 128, 256])
@pytest.mark.parametrize("activation", ["tanh", "linear"])
@pytest.mark.parametrize("n_types", [1, 3])
def test_forces_energy_virial(htf, cuda, n_types, activation, NN, dtype):
    rng = np.random.default_rng(7 + NN + 3 * n_types)
    nl, _ = random_nlist(rng, 300, NN, fill=0.75, rmin=0.3, rmax=3.4, ntypes=n_types, dtype=np.float64)
    x = torch.from_numpy(nl).to(dtype).to(cuda)
    lay = _layer(htf, K=32 if n_types == 1 else 16, n_types=n_types, H1=64, H2=48, activation=activation,
                 high=3.0, seed=5 + n_types)
    f, v = _forces(htf, lay, x)
    assert f.dtype == dtype and v.dtype == dtype and f.shape == (300, 4) and v.shape == (300, 3, 3)
    F, E, _, V = reference(lay, x)
    _close(f[:, :3], F, "forces")
    _close(f[:, 3], E, "energy")
    _close(v, V, "virial")
    # without the virial: the same forces, bit for bit
    f2 = _forces(htf, lay, x, virial=False)
    assert torch.equal(f2, f)


def test_c3_shape(htf, cuda):
    """N = 131 072, NN = 128, K = 32, one type, 64 x 64, tanh: the probe's shape, once."""
    N, NN = 131072, 128
    g = torch.Generator(device=cuda).manual_seed(31)
    cnt = torch.randint(60, NN + 1, (N, 1), device=cuda, generator=g)
    d = torch.randn((N, NN, 3), device=cuda, generator=g)
    d = d / d.norm(dim=2, keepdim=True)
    r = 0.8 + 2.4 * torch.rand((N, NN, 1), device=cuda, generator=g)
    mask = (torch.arange(NN, device=cuda)[None, :] < cnt).to(torch.float32)[..., None]
    x = torch.cat([d * r * mask, torch.zeros((N, NN, 1), device=cuda)], dim=2).contiguous()
    lay = _layer(htf, K=32, H1=64, H2=64, seed=9)
    f = _forces(htf, lay, x, virial=False)
    F, E, _, _ = reference(lay, x, virial=False)
    _close(f[:, :3], F, "forces")
    _close(f[:, 3], E, "energy")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_descriptor_stage(htf, cuda, dtype):
    rng = np.random.default_rng(12)
    nl, _ = random_nlist(rng, 200, 128, fill=0.8, rmin=0.2, rmax=3.5, ntypes=3, dtype=np.float64)
    x = torch.from_numpy(nl).to(dtype).to(cuda)
    lay = _layer(htf, K=20, n_types=3, low=0.5, high=2.5)
    G = lay.descriptor(x)
    assert G.shape == (200, 60) and G.dtype == dtype
    _, _, Gref, _ = reference(lay, x, virial=False)
    _close(G, Gref, "descriptor")
    # it is what the network reads: E from the descriptor by the same Dense stack in fp64 agrees
    W = [torch.as_tensor(w.astype(np.float64), device=cuda) for w in lay.get_weights()]
    e = (torch.tanh(torch.tanh(G.double() @ W[0] + W[1]) @ W[2] + W[3]) @ W[4] + W[5])[:, 0]
    _close(_forces(htf, lay, x, virial=False)[:, 3], e, "energy of G")


# ------------------------------------------------------------------------------------------------ 2. edge cases
def test_edge_rows(htf, cuda):
    """Row 0: no live neighbor, padding with nonzero column 3.  Row 1: one neighbor at r = 1e4, far past `high` (its
    Gaussians underflow).  Row 2: out-of-range types (-1, 3, 7, 2.6 -> 3) beside in-range ones.  Row 3: padding slots with
    nonzero column 3 after real neighbors."""
    lay = _layer(htf, K=16, n_types=3, H1=24, H2=16)
    NN = 70
    rng = np.random.default_rng(3)
    nl = np.zeros((4, NN, 4))
    nl[0, :, 3] = 2.0
    nl[1, 0, :3] = [1e4, -2.0, 3.0]
    nl[1, 1, :3] = [0.9, 0.3, -0.2]
    nl[1, 1, 3] = 1.0
    v = rng.standard_normal((10, 3))
    nl[2, :10, :3] = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.8, 2.8, (10, 1))
    nl[2, :10, 3] = [0, 1, 2, -1, 3, 7, 2.6, 1, 0, 2]
    nl[3, :10] = nl[2, :10]
    nl[3, :10, 3] = [0, 1, 2, 0, 1, 2, 1, 1, 0, 2]
    nl[3, 10:, 3] = 1.0
    x = torch.from_numpy(nl).float().to(cuda)
    f, vir = _forces(htf, lay, x)
    assert torch.isfinite(f).all() and torch.isfinite(vir).all()
    F, E, G, V = reference(lay, x)
    _close(f[:, :3], F, "forces")
    _close(f[:, 3], E, "energy")
    _close(vir, V, "virial")
    # row 0: E = MLP(0), zero force and virial
    W = [torch.as_tensor(w.astype(np.float64), device=cuda) for w in lay.get_weights()]
    e0 = (torch.tanh(torch.tanh(W[1]) @ W[2] + W[3]) @ W[4] + W[5])[0]
    assert abs(f[0, 3].item() - e0.item()) <= 1e-6 * max(1.0, abs(e0.item()))
    assert (f[0, :3] == 0).all() and (vir[0] == 0).all()
    assert (lay.descriptor(x)[0] == 0).all()
    # row 1: the far neighbor adds nothing, exactly; the near one is all there is
    x1 = x[1:2].clone()
    x1[0, 0] = 0.0
    assert torch.equal(lay.descriptor(x[1:2]), lay.descriptor(x1))
    assert torch.equal(lay.forces(x[1:2]), lay.forces(x1))
    # row 2: the out-of-range neighbors contribute nothing
    x2 = x[2:3].clone()
    x2[0, [3, 4, 5, 6]] = 0.0
    assert torch.equal(lay.descriptor(x[2:3]), lay.descriptor(x2))
    assert torch.equal(lay.forces(x[2:3]), lay.forces(x2))
    # row 3: padding's column 3 is ignored
    x3 = x[3:4].clone()
    x3[0, 10:, 3] = 0.0
    assert torch.equal(lay.forces(x[3:4]), lay.forces(x3))


def test_one_type_ignores_column_3(htf, cuda):
    rng = np.random.default_rng(8)
    nl, _ = random_nlist(rng, 64, 64, ntypes=5, dtype=np.float32)
    x = torch.from_numpy(nl).to(cuda)
    x0 = x.clone()
    x0[:, :, 3] = 0.0
    lay = _layer(htf, K=24)
    assert torch.equal(lay.forces(x), lay.forces(x0))


def test_zero_rows(htf, cuda):
    lay = _layer(htf, K=8, n_types=2)
    for dt in (torch.float32, torch.float64):
        x = torch.zeros((0, 32, 4), dtype=dt, device=cuda)
        f, v = _forces(htf, lay, x)
        assert f.shape == (0, 4) and v.shape == (0, 3, 3) and f.dtype == dt
        assert lay.descriptor(x).shape == (0, 16)


# ------------------------------------------------------------------------------------------------ 3. the same network from the layers
def test_equals_network_written_with_the_layers(htf, cuda):
    """RBFExpansion of safe_norm, masked by nlist_rinv > 0, summed over the neighbors, three Dense layers with the layer's
    weights: the generic route (torch ops + autograd), fp32 both.  Each is held to 2e-5 of the fp64 scale (the generic route
    by tests/test_gpu_generic.py, the kernel above), so the two differ by at most twice that: 4e-5."""
    rng = np.random.default_rng(21)
    nl, _ = random_nlist(rng, 500, 96, fill=0.7, rmin=0.6, rmax=2.9, dtype=np.float32)
    lay = _layer(htf, K=16, H1=24, H2=20, low=0.5, high=2.5, seed=4)
    ws = lay.get_weights()

    class BP(htf.SimModel):
        def setup(self):
            self.rbf = htf.RBFExpansion(0.5, 2.5, 16)
            self.d1 = htf.Dense(24, activation="tanh")
            self.d2 = htf.Dense(20, activation="tanh")
            self.d3 = htf.Dense(1)
            for d, (k, b) in zip((self.d1, self.d2, self.d3), ((ws[0], ws[1]), (ws[2], ws[3]), (ws[4], ws[5]))):
                d.build(k.shape[0])
                d.set_weights([k, b])

        def compute(self, nlist, positions, box):
            r = htf.safe_norm(nlist[:, :, :3], axis=2)
            live = (htf.nlist_rinv(nlist).tensor() > 0).to(torch.float32)
            g = (self.rbf(r) * live[..., None]).sum(dim=1)
            return htf.compute_nlist_forces(nlist, self.d3(self.d2(self.d1(g)))[:, 0], virial=True)

    x = torch.from_numpy(nl).to(cuda)
    f_ref, v_ref = BP(96)([htf.Nlist(x), torch.zeros((len(nl), 4), device=cuda), torch.eye(3, device=cuda)], False)
    f, v = _forces(htf, lay, x)
    _close(f[:, :3], f_ref[:, :3].detach(), "forces", tol=2 * TOL)
    _close(f[:, 3], f_ref[:, 3].detach(), "energy", tol=2 * TOL)
    _close(v, v_ref.detach(), "virial", tol=2 * TOL)


# ------------------------------------------------------------------------------------------------ 4. determinism and weights
def test_bitwise_reproducible_and_batch_independent(htf, cuda):
    rng = np.random.default_rng(5)
    nl, _ = random_nlist(rng, 999, 128, ntypes=2, dtype=np.float32)
    x = torch.from_numpy(nl).to(cuda)
    lay = _layer(htf, K=16, n_types=2, H1=64, H2=64)
    a, va = lay.forces(x, virial=True)
    b, vb = lay.forces(x, virial=True)
    assert torch.equal(a, b) and torch.equal(va, vb)
    parts = torch.cat([lay.forces(x[s:s + 333].contiguous()) for s in range(0, 999, 333)])
    assert torch.equal(parts, a)
    assert torch.equal(lay.descriptor(x), torch.cat([lay.descriptor(x[s:s + 100].contiguous()) for s in range(0, 999, 100)]))


def test_weights_written_reach_the_next_call(htf, cuda):
    """b3 += 0.25 in place on w moves every energy by 0.25 and no force; set_weights doubling W3 doubles every force."""
    rng = np.random.default_rng(6)
    nl, _ = random_nlist(rng, 256, 64, dtype=np.float32)
    x = torch.from_numpy(nl).to(cuda)
    lay = _layer(htf, K=12, H1=16, H2=16)
    f0 = lay.forces(x)
    with torch.no_grad():
        lay.w[-1] += 0.25
    f1 = lay.forces(x)
    assert torch.equal(f1[:, :3], f0[:, :3])
    assert (f1[:, 3] - f0[:, 3] - 0.25).abs().max().item() <= 1e-6 * (1.0 + f0[:, 3].abs().max().item())
    ws = lay.get_weights()
    b3 = ws[5].copy()
    ws[4] = ws[4] * np.float32(2.0)
    lay.set_weights(ws)
    f2 = lay.forces(x)
    assert torch.equal(f2[:, :3], 2.0 * f1[:, :3])
    _close(f2[:, 3] - float(b3[0]), 2.0 * (f1[:, 3] - float(b3[0])), "energy", tol=1e-6)


# ------------------------------------------------------------------------------------------------ 5. through tfcompute
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


class _Desc:
    """Model factories sharing one set of weights."""

    def __init__(self, htf, lay):
        self.htf, self.lay = htf, lay

    def kernel_model(self):
        htf, lay = self.htf, self.lay

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

    def layers_model(self):
        htf, lay = self.htf, self.lay
        ws = lay.get_weights()

        class L(htf.SimModel):
            def setup(self):
                self.rbf = htf.RBFExpansion(lay.low, lay.high, lay.K)
                self.ds = [htf.Dense(lay.H1, activation="tanh"), htf.Dense(lay.H2, activation="tanh"), htf.Dense(1)]
                for d, (k, b) in zip(self.ds, ((ws[0], ws[1]), (ws[2], ws[3]), (ws[4], ws[5]))):
                    d.build(k.shape[0])
                    d.set_weights([k, b])

            def compute(self, nlist, positions, box):
                r = htf.safe_norm(nlist[:, :, :3], axis=2)
                live = (htf.nlist_rinv(nlist).tensor() > 0).to(torch.float32)
                g = (self.rbf(r) * live[..., None]).sum(dim=1)
                return htf.compute_nlist_forces(nlist, self.ds[2](self.ds[1](self.ds[0](g)))[:, 0])
        return L


def test_nve_through_tfcompute_tracks_the_layers_model(htf, cuda):
    """Ten NVE steps of 500 particles: the kernel model stays eager (no plan, no generic op) and tracks the same network
    written with RBFExpansion and Dense on the torch route."""
    NN = 128
    lay = _layer(htf, K=16, H1=32, H2=32, low=0.8, high=2.5, seed=14, bias=0.0)
    fac = _Desc(htf, lay)
    runs = []
    for Model in (fac.kernel_model(), fac.layers_model()):
        sim, sysm = _fcc_sim(htf, cuda, seed=17)
        model = Model(NN)
        tfc = htf.tfcompute(model)
        tfc.attach(sim.nlist_cell(), r_cut=2.5)
        sim.run(10)
        torch.cuda.synchronize()
        runs.append((model, tfc, sysm.pos[:sysm.N, :3].double().cpu().numpy(), sysm.force[:sysm.N].double().cpu().numpy()))
    (mk, tk, pk, fk), (_, _, pl, fl) = runs
    assert not tk.graph_safe() and tk._plan is None
    assert "generic" not in mk.ops and mk.ops.count("descriptor_mlp") >= 10
    assert np.abs(fl[:, :3]).max() > 1e-2
    assert np.abs(pk - pl).max() < 1e-4
    assert np.abs(fk - fl).max() <= 1e-4 * np.abs(fl).max()


def test_tfcompute_batches_give_the_same_bits(htf, cuda):
    NN = 128
    lay = _layer(htf, K=16, H1=32, H2=32, low=0.8, high=2.5, seed=15)
    M = _Desc(htf, lay).kernel_model()
    forces = []
    for bs in (None, 500 // 3):
        sim, sysm = _fcc_sim(htf, cuda, seed=19)
        tfc = htf.tfcompute(M(NN))
        tfc.attach(sim.nlist_cell(), r_cut=2.5, batch_size=bs)
        sim.run(3)
        torch.cuda.synchronize()
        forces.append((sysm.force[:sysm.N].clone(), sysm.pos[:sysm.N].clone()))
    assert torch.equal(forces[0][0], forces[1][0]) and torch.equal(forces[0][1], forces[1][1])


def test_training_raises(htf, cuda):
    import build_examples
    lay = _layer(htf, K=8, H1=8, H2=8, high=2.5)
    M = _Desc(htf, lay).kernel_model()
    sim, sysm = _fcc_sim(htf, cuda, seed=23)
    nlist = sim.nlist_cell()
    lj = htf.tfcompute(build_examples.LJModel(128))
    lj.attach(nlist, r_cut=2.5)
    model = M(128, output_forces=False)
    model.compile(htf.optimizers.Adam(0.01), loss='MeanSquaredError')
    tfc = htf.tfcompute(model)
    tfc.attach(nlist, train=True, r_cut=2.5)
    tfc.set_reference_forces(lj)
    with pytest.raises(NotImplementedError, match="DescriptorMLP"):
        sim.run(1)
