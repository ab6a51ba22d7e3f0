"""htf.DescriptorMLP(conservative=True) on the MI355X (csrc/cforce.hip, include/htf_cforce.h): the forces of the total energy,
F = -d(sum_i E_i)/dr, against fp64 torch autograd of the definition

    x_ij = minimum image of pos[idx[i, s]] - pos[i],  r_ij = sqrt(sum_c (x_ij,c + 1e-7)^2),  live = r_ij > 3e-6 (and r_ij < rc)
    t_ij = 0 (n_types = 1) or the type of particle idx[i, s]
    G_i[t*K + k] = sum_s live [t_ij = t] fc(r_ij) exp(-(r_ij - mu_k)^2 / gap),   fc = 0.5 (cos(pi r / rc) + 1) or 1
    E_i = W3^T act(W2^T act(W1^T G_i + b1) + b2) + b3,   F = -grad(sum_i E_i, pos)

and, for the virial and the slots whose reverse term is dropped, against the fp64 formula of include/htf_cforce.h.

Configurations: a simple-cubic lattice of spacing 1 with uniform jitter in [-0.05, 0.05]^3, so that list symmetry follows
from geometry (any pair distance moves by at most 0.174): (a) 6^3 particles, list cutoff 1.8, at most 26 neighbors in NN = 37;
(b) 7^3 particles, list cutoff 2.9, at most 122 neighbors in NN = 128, and in NN = 256 for four slots per lane.  The jitter is
rounded to multiples of 2^-12: coordinate differences are then exact in fp32, and the fp32 pair vectors of compute_nlist ARE
the oracle's (asserted), so the comparison measures the kernels' arithmetic and nothing else.

Bound: TOL = 2e-5 of the largest reference value, the project's bound for this arithmetic (test_gpu_desc.py)."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 2e-5

CONFIGS = {"a": (6, 1.8, 37), "b": (7, 2.9, 128), "b256": (7, 2.9, 256)}


# ------------------------------------------------------------------------------------------------ systems and layers
@functools.lru_cache(maxsize=None)
def _system(name):
    """(pos [N, 4] fp64 with the type in column 3, L, list cutoff, x [N, NN, 4] fp32 with the neighbors' types, idx [N, NN] int32),
    all on the device; the list by compute_nlist(sorted=True), whose return_types=False call gives the index of the same slots."""
    import hoomd_tf_amd as htf
    n, rc_list, NN = CONFIGS[name]
    rng = np.random.default_rng(40 + n)
    ijk = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    pos = ijk + np.round(rng.uniform(-0.05, 0.05, ijk.shape) * 4096.0) / 4096.0
    types = rng.integers(0, 3, len(pos)).astype(np.float64)
    p = torch.from_numpy(np.concatenate([pos, types[:, None]], axis=1)).cuda()
    L = float(n)
    p32 = p.to(torch.float32)
    assert torch.equal(p32.double(), p)
    x = htf.compute_nlist(p32, rc_list, NN, [L, L, L], sorted=True, return_types=True).detach()
    idx = torch.round(htf.compute_nlist(p32, rc_list, NN, [L, L, L], sorted=True, return_types=False).detach()[:, :, 3]).to(torch.int32)
    occ = (x[:, :, :3] != 0).any(dim=2)
    # preconditions: no row overflows (every row has an empty slot), and the slots of the two calls are the same particles
    assert bool((~occ).any(dim=1).all())
    assert torch.equal(_pair_vectors(p[:, :3], idx, occ, L), x[:, :, :3].double())
    assert torch.equal(p[:, 3][idx.long()][occ], x[:, :, 3].double()[occ])
    return p, L, rc_list, x.contiguous(), idx.contiguous()


def _pair_vectors(pos, idx, occ, L):
    d = pos[idx.long()] - pos[:, None, :]
    d = d - L * torch.round(d / L)
    return d * occ[..., None].to(d.dtype)


def _layer(htf, K=16, n_types=1, activation="tanh", high=1.8, r_cut=None, n_species=1, seed=3, H1=32, H2=24, bias=0.1):
    lay = htf.DescriptorMLP(K=K, H1=H1, H2=H2, low=0.5, high=high, n_types=n_types, activation=activation, seed=seed,
                            r_cut=r_cut, n_species=n_species, conservative=True)
    rng = np.random.default_rng(seed + 100)   # (mlp_params' zero biases would leave the bias paths untested)
    ws = lay.get_weights()
    for i in (1, 3, 5):
        ws[i] = (bias * rng.standard_normal(ws[i].shape)).astype(np.float32)
    lay.set_weights(ws)
    return lay


# ------------------------------------------------------------------------------------------------ the fp64 oracle
def _weights(lay, dev):
    W = [torch.as_tensor(np.asarray(w, dtype=np.float64), device=dev) for w in lay.get_weights()]
    return W if lay.n_species > 1 else [w[None] for w in W]


def _descriptor(lay, x3, tn):
    """(G [B, D], r, live, fc, fc') of pair vectors x3 [B, NN, 3] fp64 and neighbor types tn [B, NN]."""
    mu = torch.as_tensor(lay.centers.astype(np.float64), device=x3.device)
    t = x3 + 1e-7
    r = torch.sqrt((t * t).sum(dim=2))
    live = r > 3e-6
    fc, dfc = torch.ones_like(r), torch.zeros_like(r)
    if lay.r_cut is not None:
        live = live & (r < lay.r_cut)
        fc = 0.5 * (torch.cos(math.pi * r / lay.r_cut) + 1.0)
        dfc = -0.5 * (math.pi / lay.r_cut) * torch.sin(math.pi * r / lay.r_cut)
    e = torch.exp(-(r[..., None] - mu) ** 2 / float(lay.gap)) * (fc * live.to(r.dtype))[..., None]
    G = torch.cat([(e * (tn == tt).to(r.dtype)[..., None]).sum(dim=1) for tt in range(lay.n_types)], dim=1)
    return G, r, live, fc, dfc


def _network(lay, G, sp):
    W = _weights(lay, G.device)
    act = torch.tanh if lay.activation == "tanh" else (lambda v: v)
    h1 = act(torch.einsum("bd,bdh->bh", G, W[0][sp]) + W[1][sp])
    h2 = act(torch.einsum("bd,bdh->bh", h1, W[2][sp]) + W[3][sp])
    return torch.einsum("bd,bdh->bh", h2, W[4][sp])[:, 0] + W[5][sp][:, 0]


def _neighbor_types(lay, x):
    return torch.round(x[:, :, 3].double()) if lay.n_types > 1 else torch.zeros(x.shape[:2], dtype=torch.float64, device=x.device)


def oracle(lay, pos, L, x, idx, sp=None):
    """Autograd of the definition: (F [N, 3] = -grad(sum E, pos), E [N])."""
    occ = (x[:, :, :3] != 0).any(dim=2)
    sp = torch.zeros(len(pos), dtype=torch.long, device=pos.device) if sp is None else sp
    q = pos[:, :3].detach().clone().requires_grad_(True)
    G = _descriptor(lay, _pair_vectors(q, idx, occ, L), _neighbor_types(lay, x))[0]
    E = _network(lay, G, sp)
    (g,) = torch.autograd.grad(E.sum(), q)
    return -g, E.detach()


def formula(lay, x, idx, ti, sp=None):
    """The header's formula in fp64 on the tensor itself: (F [B, 3], E [B], W [B, 3, 3], sum |x . phi|, dE_total/d(eps)).  ``ti``:
    the rows' own types (long); a slot whose index is outside [0, B), or a row whose type is out of range, has no reverse term."""
    B = x.shape[0]
    T, K = lay.n_types, lay.K
    mu = torch.as_tensor(lay.centers.astype(np.float64), device=x.device)
    sp = torch.zeros(B, dtype=torch.long, device=x.device) if sp is None else sp
    x3 = x[:, :, :3].double()
    tn = _neighbor_types(lay, x)
    eps = torch.zeros((), dtype=torch.float64, device=x.device, requires_grad=True)
    (dE_deps,) = torch.autograd.grad(_network(lay, _descriptor(lay, x3 * (1.0 + eps), tn)[0], sp).sum(), eps)
    G, r, live, fc, dfc = _descriptor(lay, x3, tn)
    G = G.detach().requires_grad_(True)
    E = _network(lay, G, sp)
    (g,) = torch.autograd.grad(E.sum(), G)
    g = g.view(B, T, K)
    tnc = tn.long().clamp(0, T - 1)
    gi = g[torch.arange(B, device=x.device)[:, None], tnc] * ((tn >= 0) & (tn < T)).to(g.dtype)[..., None]
    j = idx.long()
    rev = live & (j >= 0) & (j < B) & ((ti >= 0) & (ti < T))[:, None]
    gj = g[j.clamp(0, B - 1), ti.clamp(0, T - 1)[:, None]] * rev.to(g.dtype)[..., None]
    s = gi + gj
    d = r[..., None] - mu
    ek = torch.exp(-d * d / float(lay.gap))
    dEdr = fc * (-2.0 / float(lay.gap)) * (s * d * ek).sum(dim=-1) + dfc * (s * ek).sum(dim=-1)
    phi = (dEdr / r * live.to(r.dtype))[..., None] * (x3 + 1e-7)
    W = -0.5 * torch.einsum("bsi,bsj->bij", x3, phi)
    return phi.sum(dim=1), E.detach(), W, (x3 * phi).sum(dim=-1).abs().sum(), dE_deps


def _close(got, ref, what, tol=TOL, scale=None):
    got, ref = got.double(), ref.double()
    scale = ref.abs().max().item() if scale is None else float(scale)
    err = (got - ref).abs().max().item()
    print("%s: max err %.3g, scale %.3g, ratio %.3g" % (what, err, scale, err / scale if scale else float("nan")))
    assert np.isfinite(err) and err <= tol * scale, "%s: max err %.3g of scale %.3g" % (what, err, scale)


def _run(htf, lay, p, x, idx, virial=False):
    """Through the public route: compute_nlist_forces of layer(nlist, positions) on a list that carries its index."""
    nl = htf.Nlist(x, index=idx)
    return htf.compute_nlist_forces(nl, lay(nl, p.to(x.dtype)), virial=virial)


# ------------------------------------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("config", ["a", "b", "b256"])
@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("activation", ["tanh", "linear"])
@pytest.mark.parametrize("n_types", [1, 3])
def test_forces_and_energy(htf, cuda, n_types, activation, cut, config, dtype):
    """K = 16 with one type (the gather reads float4), K = 10 with three (it reads single floats)."""
    p, L, rc_list, x, idx = _system(config)
    lay = _layer(htf, K=16 if n_types == 1 else 10, n_types=n_types, activation=activation, high=rc_list,
                 r_cut=0.9 * rc_list if cut else None, seed=5 + n_types)
    xx = x.to(dtype)
    f = _run(htf, lay, p, xx, idx)
    assert f.dtype == dtype and f.shape == (len(p), 4)
    F, E = oracle(lay, p, L, x, idx)
    assert F.abs().max().item() > 1e-3
    _close(f[:, :3], F, "forces")
    _close(f[:, 3], E, "energy")
    # the energy column is the row operator's, bit for bit
    assert torch.equal(f[:, 3], lay.forces(xx)[:, 3])


def test_one_network_per_species(htf, cuda):
    """n_species = 2 over a system of three types with n_types = 2: type-2 particles are in nobody's descriptor, their own
    rows still pull on their neighbors."""
    p, L, rc_list, x, idx = _system("a")
    lay = _layer(htf, K=20, n_types=2, high=rc_list, r_cut=0.9 * rc_list, n_species=2, seed=11)
    sp = (p[:, 3].long() % 2)
    f = lay.total_forces(x, idx, types=p[:, 3].contiguous(), species=sp.to(torch.float32))
    F, E = oracle(lay, p, L, x, idx, sp=sp)
    _close(f[:, :3], F, "forces")
    _close(f[:, 3], E, "energy")
    assert torch.equal(f[:, 3], lay.forces(x, species=sp.to(torch.float32))[:, 3])


# ------------------------------------------------------------------------------------------------ 2. momentum
@pytest.mark.parametrize("config", ["a", "b"])
def test_momentum(htf, cuda, config):
    """Every row is within TOL max|F| of the gradient, whose rows sum to zero exactly: |sum_i F_i| <= TOL N max|F| at worst.
    The row operator's forces on the same input are not the gradient of anything and break that bound."""
    p, L, rc_list, x, idx = _system(config)
    lay = _layer(htf, K=16, n_types=3, high=rc_list, r_cut=0.9 * rc_list, seed=21)
    f = _run(htf, lay, p, x, idx)[:, :3].double()
    bound = TOL * len(p) * f.abs().max().item()
    total = f.sum(dim=0).abs().max().item()
    print("sum F %.3g, bound %.3g" % (total, bound))
    assert total <= bound
    row = lay.forces(x)[:, :3].double()
    assert row.sum(dim=0).abs().max().item() > TOL * len(p) * row.abs().max().item()


# ------------------------------------------------------------------------------------------------ 3. virial
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("config,cut", [("a", True), ("b", False), ("b256", True)])
def test_virial(htf, cuda, config, cut, dtype):
    p, L, rc_list, x, idx = _system(config)
    lay = _layer(htf, K=16, n_types=3, high=rc_list, r_cut=0.9 * rc_list if cut else None, seed=31)
    xx = x.to(dtype)
    f, w = _run(htf, lay, p, xx, idx, virial=True)
    assert w.dtype == dtype and w.shape == (len(p), 3, 3)
    F, E, W, xphi, dE_deps = formula(lay, x, idx, p[:, 3].long())
    _close(f[:, :3], F, "forces")
    _close(w, W, "virial")
    # the trace of the total is the volume derivative of the total energy
    _close(w.double().diagonal(dim1=1, dim2=2).sum().reshape(1), -dE_deps.reshape(1), "trace", scale=xphi.item())
    # without the virial: the same forces, bit for bit
    assert torch.equal(_run(htf, lay, p, xx, idx), f)


# ------------------------------------------------------------------------------------------------ 4. bits and edges
def test_bits(htf, cuda):
    p, L, rc_list, x, idx = _system("a")
    lay = _layer(htf, K=6, n_types=3, high=rc_list, r_cut=0.9 * rc_list, seed=41)
    types = p[:, 3].contiguous()
    a, va = lay.total_forces(x, idx, virial=True, types=types)
    b, vb = lay.total_forces(x, idx, virial=True, types=types)
    assert torch.equal(a, b) and torch.equal(va, vb)
    # row i with two live slots, pointing at j1 and j2: the same bits in the batch of (i, j1, j2) with the indices remapped
    i = 100
    x2, idx2 = x.clone(), idx.clone()
    x2[i, 2:] = 0.0
    j1, j2 = int(idx[i, 0]), int(idx[i, 1])
    full = lay.total_forces(x2, idx2, virial=True, types=types)
    rows = torch.tensor([i, j1, j2], device=cuda)
    remap = torch.full((len(p),), -1, dtype=torch.int32, device=cuda)
    remap[rows] = torch.arange(3, dtype=torch.int32, device=cuda)
    sub = lay.total_forces(x2[rows].contiguous(), remap[idx2[rows].long()].contiguous(), virial=True, types=types[rows].contiguous())
    assert full[0][i, :3].abs().max().item() > 0
    assert torch.equal(sub[0][0], full[0][i]) and torch.equal(sub[1][0], full[1][i])


def test_edges(htf, cuda):
    """Indices outside [0, B) on live slots drop that slot's reverse term and nothing else; a float index tensor is taken by
    rint; a row of empty slots has no force and the energy of G = 0; a row whose own type is out of range gathers nothing."""
    p, L, rc_list, x, idx = _system("a")
    B = len(p)
    lay = _layer(htf, K=16, n_types=3, high=rc_list, seed=51)
    x, idx, types = x.clone(), idx.clone(), p[:, 3].clone()
    idx[0, 0], idx[1, 0], idx[2, 1], idx[3, 2] = -1, B, B + 5, -7
    x[5] = 0.0            # (its neighbors still read g_5 = dE/dG at G = 0)
    types[7] = 3.0        # out of range: row 7 has forward terms only
    f, w = lay.total_forces(x, idx, virial=True, types=types)
    assert torch.isfinite(f).all() and torch.isfinite(w).all()
    F, E, W, _, _ = formula(lay, x, idx, types.long())
    _close(f[:, :3], F, "forces")
    _close(f[:, 3], E, "energy")
    _close(w, W, "virial")
    # the dropped terms are not small: with them the answer is different
    Fall = formula(lay, x, _system("a")[4], types.long())[0]
    assert (Fall[:4] - F[:4]).abs().max().item() > 100 * TOL * F.abs().max().item()
    assert torch.equal(lay.total_forces(x, idx.to(torch.float32) + 0.25, virial=True, types=types)[0], f)
    assert (f[5, :3] == 0).all() and (w[5] == 0).all()
    e0 = _network(lay, torch.zeros((1, lay.D), dtype=torch.float64, device=cuda), torch.zeros(1, dtype=torch.long, device=cuda))
    assert abs(f[5, 3].item() - e0.item()) <= 1e-6 * max(1.0, abs(e0.item()))


def test_zero_rows(htf, cuda):
    lay = _layer(htf, K=8, n_types=2)
    for dt in (torch.float32, torch.float64):
        x = torch.zeros((0, 32, 4), dtype=dt, device=cuda)
        f, v = lay.total_forces(x, torch.zeros((0, 32), dtype=torch.int32, device=cuda), virial=True,
                                types=torch.zeros((0,), device=cuda))
        assert f.shape == (0, 4) and v.shape == (0, 3, 3) and f.dtype == dt


# ------------------------------------------------------------------------------------------------ 5. the index tensor
def _fcc(cuda, seed, types=None):
    from hoomd_tf_amd import standin
    pos, L, a = standin.fcc_positions(5, 0.8442)
    rng = np.random.default_rng(seed)
    pos = pos + 0.03 * a * rng.standard_normal(pos.shape)
    pos -= np.round(pos / L) * L
    return standin.System(pos, L, types=types, dtype=torch.float32, device=cuda), float(L[0])


@pytest.mark.parametrize("NN", [128, 8])
def test_pair_index(htf, cuda, NN):
    """NN = 8: every row overflows (about 55 neighbors within 2.5), so the wrap decides every slot."""
    from hoomd_tf_amd import ops, standin
    sysm, L = _fcc(cuda, 61, types=np.arange(500) % 3)
    nl = standin.CellNlist(sysm, r_cut=2.5, r_buff=0.4)
    nl.build()
    pv = ops.build_pair_vectors(sysm.pos, nl.n_neigh, nl.head_list, nl.nlist, sysm.box, 2.5, NN, n_local=sysm.N)
    idx = ops.build_pair_index(sysm.pos, nl.n_neigh, nl.head_list, nl.nlist, sysm.box, 2.5, NN, n_local=sysm.N)
    assert idx.shape == (500, NN) and idx.dtype == torch.int32
    assert torch.equal(idx, ops.build_pair_index(sysm.pos, nl.n_neigh, nl.head_list, nl.nlist, sysm.box, 2.5, NN, n_local=sysm.N))
    occ = (pv != 0).any(dim=2)
    assert bool(occ.all()) == (NN == 8) and int(occ.sum()) >= 500 * min(NN, 40)
    assert (idx[~occ] == -1).all()
    assert ((idx[occ] >= 0) & (idx[occ] < 500)).all()
    pos = sysm.pos[:500, :3].double()
    d = pos[idx.clamp(min=0).long()] - pos[:, None, :]
    d = d - L * torch.round(d / L)
    assert ((d - pv[:, :, :3].double()).abs()[occ]).max().item() <= 1e-6 * L
    own = sysm.pos[:500, 3].contiguous().view(torch.int32)
    assert torch.equal(own[idx.clamp(min=0).long()][occ].to(torch.float32), pv[:, :, 3][occ])
    # a batch of the rows: the same slots
    part = ops.build_pair_index(sysm.pos, nl.n_neigh, nl.head_list, nl.nlist, sysm.box, 2.5, NN, offset=100, batch_size=150,
                                n_local=sysm.N)
    assert torch.equal(part, idx[100:250])


# ------------------------------------------------------------------------------------------------ 6. through tfcompute
def _sim(htf, cuda, seed):
    from hoomd_tf_amd import standin
    sysm, L = _fcc(cuda, seed)
    sysm.randomize_velocities(kT=0.3, seed=seed)
    sim = standin.Simulation(sysm)
    sim.integrate_nve(0.001)
    return sim, sysm, L


def _model(htf, lay, with_positions=True):
    class M(htf.SimModel):
        def setup(self):
            self.desc = lay
            self.seen = None

        def compute(self, nlist, positions, box):
            self.seen = positions.detach().clone()
            return htf.compute_nlist_forces(nlist, self.desc(nlist, positions) if with_positions else self.desc(nlist))
    return M


def test_nve_through_tfcompute(htf, cuda):
    """Five NVE steps of 500 particles.  The last forces equal the all-pairs fp64 gradient at the positions they were
    evaluated at: every pair within the layer's r_cut = 2.0 under minimum image, no list and no index -- valid because fc
    vanishes before the list's cutoff 2.5.  Momentum: each step adds dt sum_i F_i, at most dt TOL N max|F| (test_momentum),
    and each of the N fp32 updates v += f dt rounds once, by at most 2^-24 max|v| (half an ulp)."""
    steps, dt = 5, 0.001
    lay = _layer(htf, K=16, high=2.0, r_cut=2.0, seed=71)
    sim, sysm, L = _sim(htf, cuda, 73)
    model = _model(htf, lay)(128)
    tfc = htf.tfcompute(model)
    tfc.attach(sim.nlist_cell(), r_cut=2.5)
    p0 = sysm.vel[:sysm.N, :3].double().sum(dim=0)
    sim.run(steps)
    torch.cuda.synchronize()
    assert tfc._plan is None and not tfc.graph_safe()
    f = sysm.force[:sysm.N].double()
    q = model.seen[:, :3].double().requires_grad_(True)
    d = q[None, :, :] - q[:, None, :]
    d = d - L * torch.round(d.detach() / L)
    off = ~torch.eye(sysm.N, dtype=torch.bool, device=cuda)
    x3 = d * off[..., None].to(d.dtype)
    G = _descriptor(lay, x3, torch.zeros((sysm.N, sysm.N), dtype=torch.float64, device=cuda))[0]
    E = _network(lay, G, torch.zeros(sysm.N, dtype=torch.long, device=cuda))
    (g,) = torch.autograd.grad(E.sum(), q)
    assert g.abs().max().item() > 1e-2
    _close(f[:, :3], -g, "forces")
    _close(f[:, 3], E.detach(), "energy")
    dp = (sysm.vel[:sysm.N, :3].double().sum(dim=0) - p0).abs().max().item()
    vmax, fmax = sysm.vel[:sysm.N, :3].abs().max().item(), g.abs().max().item()
    bound = steps * sysm.N * (2.0 ** -24 * vmax + dt * TOL * fmax)
    print("momentum drift %.3g, bound %.3g" % (dp, bound))
    assert dp <= bound


# ------------------------------------------------------------------------------------------------ 7. what raises
def test_raises(htf, cuda):
    with pytest.raises(ValueError, match="conservative"):
        htf.DescriptorMLP(K=8, H1=8, H2=8, conservative=True, trainable=True)
    p, L, rc_list, x, idx = _system("a")
    lay = _layer(htf, K=8, n_types=1, high=rc_list)
    with pytest.raises(ValueError, match="index"):
        nl = htf.Nlist(x)
        htf.compute_nlist_forces(nl, lay(nl))
    lay3 = _layer(htf, K=8, n_types=3, high=rc_list)
    with pytest.raises(ValueError, match="types"):
        nl = htf.Nlist(x, index=idx)
        htf.compute_nlist_forces(nl, lay3(nl))
    with pytest.raises(ValueError, match="types"):
        lay3.total_forces(x, idx)
    # batches: g_j of a neighbor in another batch does not exist yet
    sim, sysm, _ = _sim(htf, cuda, 83)
    tfc = htf.tfcompute(_model(htf, _layer(htf, K=8, high=2.0, r_cut=2.0))(128))
    tfc.attach(sim.nlist_cell(), r_cut=2.5, batch_size=sysm.N // 3)
    with pytest.raises(ValueError, match="batch"):
        sim.run(1)
    # several types through tfcompute without the positions
    sim, sysm, _ = _sim(htf, cuda, 85)
    tfc = htf.tfcompute(_model(htf, _layer(htf, K=8, n_types=3, high=2.0, r_cut=2.0), with_positions=False)(128))
    tfc.attach(sim.nlist_cell(), r_cut=2.5)
    with pytest.raises(ValueError, match="types"):
        sim.run(1)
