"""htf.DescriptorMLP(conservative=True, l_max=1 or 2) on the MI355X (csrc/angular.hip, include/htf_angular.h): the forces of the
total energy with angular channels, F = -d(sum_i E_i)/dr, against fp64 torch autograd of the definition

    x_ij = minimum image of pos[idx[i, s]] - pos[i],  r_ij = sqrt(sum_c (x_ij,c + 1e-7)^2),  u_ij = (x_ij + 1e-7) / r_ij
    live = r_ij > 3e-6 (and r_ij < rc),  t_ij = 0 (n_types = 1) or the type of particle idx[i, s]
    w_k = fc(r_ij) exp(-(r_ij - mu_k)^2 / gap),   fc = 0.5 (cos(pi r / rc) + 1) or 1
    G_i[t*K + k] = sum_s live [t_ij = t] w_k,   v_i = sum_s ... w_k u_ij,   M_i = sum_s ... w_k u_ij (outer) u_ij
    A_i = |v_i|^2,   Q_i = ||M_i||_F^2,   E_i = network([G | A | Q][: D]),   F = -grad(sum_i E_i, pos)

and, for the virial and the slots whose reverse terms are dropped, against the fp64 formula of include/htf_angular.h.

Configurations (tests/test_gpu_desc_total.py): a simple-cubic lattice of spacing 1 with uniform jitter in [-0.05, 0.05]^3 rounded
to multiples of 2^-12, so that list symmetry follows from geometry and the fp32 pair vectors of compute_nlist ARE the oracle's
(asserted): (a) 6^3 particles, list cutoff 1.8, NN = 37; (b256) 7^3 particles, list cutoff 2.9, NN = 256, four slots per lane.

Bound.  TOL = 2e-5 of the largest reference value is the project's bound for this arithmetic.  A and Q are sums of squares of
partly cancelling moments, and what fp32 costs there is a property of the definition, not of the kernel: every value test also
evaluates the same definition with torch in fp32 (autograd, on the device) and allows max(TOL, 4 x that twin's error) -- the
factor 4 of test_gpu_desc_train.py.  Both errors are printed before anything is asserted."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 2e-5

CONFIGS = {"a": (6, 1.8, 37), "b256": (7, 2.9, 256)}


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


def _layer(htf, K=16, n_types=1, activation="tanh", high=1.8, r_cut=None, n_species=1, seed=3, H1=32, H2=24, bias=0.1, l_max=1):
    lay = htf.DescriptorMLP(K=K, H1=H1, H2=H2, low=0.5, high=high, n_types=n_types, activation=activation, seed=seed,
                            r_cut=r_cut, n_species=n_species, conservative=True, l_max=l_max)
    rng = np.random.default_rng(seed + 100)   # (mlp_params' zero biases would leave the bias paths untested)
    ws = lay.get_weights()
    for i in (1, 3, 5):
        ws[i] = (bias * rng.standard_normal(ws[i].shape)).astype(np.float32)
    # Q = ||M||_F^2 is about G^2 / 3 (M is near G / 3 times the identity on a lattice), in the hundreds with 122 neighbors: the
    # Q rows of W1 are scaled so that tanh does not saturate (saturated, the fp64 gradient is exactly zero and tests nothing)
    ws[0][2 * lay.Dr:] *= np.float32(1.0 / 64.0)
    lay.set_weights(ws)
    return lay


# ------------------------------------------------------------------------------------------------ the definition, in any dtype
def _weights(lay, dev, dtype=torch.float64):
    W = [torch.as_tensor(np.asarray(w, dtype=np.float64), device=dev).to(dtype) for w in lay.get_weights()]
    return W if lay.n_species > 1 else [w[None] for w in W]


def _inputs(lay, x3, tn):
    """([G | A | Q] [B, D], aux) of pair vectors x3 [B, NN, 3] and neighbor types tn [B, NN], in x3's dtype.  aux: r, live, fc,
    fc', u [B, NN, 3], v [B, Dr, 3], M [B, Dr, 9]."""
    dt = x3.dtype
    B, NN = x3.shape[:2]
    mu = torch.as_tensor(lay.centers.astype(np.float64), device=x3.device).to(dt)
    t = x3 + 1e-7
    r = torch.sqrt((t * t).sum(dim=2))
    u = t / r[..., None]
    live = r > 3e-6
    fc, dfc = torch.ones_like(r), torch.zeros_like(r)
    if lay.r_cut is not None:
        live = live & (r < lay.r_cut)
        fc = 0.5 * (torch.cos(math.pi * r / lay.r_cut) + 1.0)
        dfc = -0.5 * (math.pi / lay.r_cut) * torch.sin(math.pi * r / lay.r_cut)
    e = torch.exp(-(r[..., None] - mu) ** 2 / float(lay.gap)) * (fc * live.to(dt))[..., None]          # [B, NN, K]
    onehot = torch.stack([(tn == tt).to(dt) for tt in range(lay.n_types)], dim=2)                     # [B, NN, T]
    et = (e[:, :, None, :] * onehot[:, :, :, None]).reshape(B, NN, lay.n_types * lay.K).transpose(1, 2)   # [B, Dr, NN]
    G = et.sum(dim=2)
    v = et @ u
    M = et @ (u[..., :, None] * u[..., None, :]).reshape(B, NN, 9)
    blocks = [G, (v * v).sum(dim=2), (M * M).sum(dim=2)][:1 + lay.l_max]
    return torch.cat(blocks, dim=1), dict(r=r, live=live, fc=fc, dfc=dfc, u=u, v=v, M=M)


def _network(lay, X, sp):
    W = _weights(lay, X.device, X.dtype)
    act = torch.tanh if lay.activation == "tanh" else (lambda v: v)
    h1 = act(torch.einsum("bd,bdh->bh", X, W[0][sp]) + W[1][sp])
    h2 = act(torch.einsum("bd,bdh->bh", h1, W[2][sp]) + W[3][sp])
    return torch.einsum("bd,bdh->bh", h2, W[4][sp])[:, 0] + W[5][sp][:, 0]


def _neighbor_types(lay, x):
    return torch.round(x[:, :, 3].double()) if lay.n_types > 1 else torch.zeros(x.shape[:2], dtype=torch.float64, device=x.device)


def oracle(lay, pos, L, x, idx, sp=None, dtype=torch.float64):
    """Autograd of the definition from the positions through minimum image: (F [N, 3] = -grad(sum E, pos), E [N]).  fp64 is the
    oracle; dtype=torch.float32 is its twin, the same arithmetic at the kernels' precision."""
    occ = (x[:, :, :3] != 0).any(dim=2)
    sp = torch.zeros(len(pos), dtype=torch.long, device=pos.device) if sp is None else sp
    q = pos[:, :3].detach().to(dtype).clone().requires_grad_(True)
    X = _inputs(lay, _pair_vectors(q, idx, occ, L), _neighbor_types(lay, x))[0]
    E = _network(lay, X, sp)
    (g,) = torch.autograd.grad(E.sum(), q)
    return -g.detach(), E.detach()


def formula(lay, x, idx, ti, sp=None):
    """The header's formula in fp64 on the tensor itself: (F [B, 3], E [B], W [B, 3, 3], sum |x . phi|, dE_total/d(eps)).  ``ti``:
    the rows' own types (long); a slot whose index is outside [0, B), or a row whose type is out of range, has no reverse terms;
    a neighbor type out of range empties the slot's own-row terms."""
    B = x.shape[0]
    T, K, Dr, lm = lay.n_types, lay.K, lay.n_types * lay.K, lay.l_max
    dev = x.device
    mu = torch.as_tensor(lay.centers.astype(np.float64), device=dev)
    sp = torch.zeros(B, dtype=torch.long, device=dev) if sp is None else sp
    ti = torch.zeros_like(ti) if T == 1 else ti   # (one type: the rows' own types are not read)
    x3 = x[:, :, :3].double()
    tn = _neighbor_types(lay, x)
    eps = torch.zeros((), dtype=torch.float64, device=dev, requires_grad=True)
    (dE_deps,) = torch.autograd.grad(_network(lay, _inputs(lay, x3 * (1.0 + eps), tn)[0], sp).sum(), eps)
    X, a = _inputs(lay, x3, tn)
    X = X.detach().requires_grad_(True)
    E = _network(lay, X, sp)
    (g,) = torch.autograd.grad(E.sum(), X)
    r, live, fc, dfc, u = a["r"], a["live"], a["fc"], a["dfc"], a["u"]
    g0 = g[:, :Dr].view(B, T, K)
    p = (2.0 * g[:, Dr:2 * Dr, None] * a["v"]).view(B, T, K, 3)
    S = (2.0 * g[:, 2 * Dr:3 * Dr, None] * a["M"]).view(B, T, K, 3, 3) if lm == 2 else torch.zeros((B, T, K, 3, 3), dtype=torch.float64, device=dev)
    rows = torch.arange(B, device=dev)[:, None]
    own = ((tn >= 0) & (tn < T)).to(torch.float64)
    tnc = tn.long().clamp(0, T - 1)
    j = idx.long()
    rev = (live & (j >= 0) & (j < B) & ((ti >= 0) & (ti < T))[:, None]).to(torch.float64)
    jc, tic = j.clamp(0, max(B - 1, 0)), ti.clamp(0, T - 1)[:, None]
    s0 = g0[rows, tnc] * own[..., None] + g0[jc, tic] * rev[..., None]                                  # [B, NN, K]
    dp = p[rows, tnc] * own[..., None, None] - p[jc, tic] * rev[..., None, None]                        # [B, NN, K, 3]
    sS = S[rows, tnc] * own[..., None, None, None] + S[jc, tic] * rev[..., None, None, None]            # [B, NN, K, 3, 3]
    d = r[..., None] - mu
    ek = torch.exp(-d * d / float(lay.gap))
    w = fc[..., None] * ek
    wp = fc[..., None] * (-2.0 / float(lay.gap)) * d * ek + dfc[..., None] * ek
    uk = u[:, :, None, :]
    dpu = (dp * uk).sum(dim=-1)
    Su = torch.einsum("bskij,bsj->bski", sS, u)
    uSu = (Su * uk).sum(dim=-1)
    radial = (wp * (s0 + dpu + uSu)).sum(dim=-1)
    tang = (w[..., None] * ((dp - dpu[..., None] * uk) + 2.0 * (Su - uSu[..., None] * uk))).sum(dim=2) / r[..., None]
    phi = (radial[..., None] * u + tang) * live.to(torch.float64)[..., None]
    W = -0.5 * torch.einsum("bsi,bsj->bij", x3, phi)
    return phi.sum(dim=1), E.detach(), W, (x3 * phi).sum(dim=-1).abs().sum(), dE_deps


def _close(got, ref, what, tol=TOL, scale=None):
    got, ref = got.double(), ref.double()
    scale = ref.abs().max().item() if scale is None else float(scale)
    err = (got - ref).abs().max().item()
    print("%s: max err %.3g, scale %.3g, ratio %.3g, bound %.3g" % (what, err, scale, err / scale if scale else float("nan"), tol))
    assert np.isfinite(err) and err <= tol * scale, "%s: max err %.3g of scale %.3g" % (what, err, scale)


def _close_twin(got, ref, twin, what):
    """Kernel and fp32 twin against the fp64 reference, both printed; the bound is max(TOL, 4 x the twin's error)."""
    ref = ref.double()
    scale = ref.abs().max().item()
    kern = (got.double() - ref).abs().max().item() / scale
    tw = (twin.double() - ref).abs().max().item() / scale
    bound = max(TOL, 4.0 * tw)
    print("%s: kernel %.3g, fp32 twin %.3g of scale %.3g; bound %.3g" % (what, kern, tw, scale, bound))
    return None if (np.isfinite(kern) and kern <= bound) else "%s: kernel error %.3g over %.3g (twin %.3g)" % (what, kern, bound, tw)


def _assert_values(f, ref, twin, what=""):
    bad = [m for m in (_close_twin(f[:, :3], ref[0], twin[0], what + "forces"), _close_twin(f[:, 3], ref[1], twin[1], what + "energy")) if m]
    assert not bad, bad


def _run(htf, lay, p, x, idx, virial=False):
    """Through the public route: compute_nlist_forces of layer(nlist, positions) on a list that carries its index."""
    nl = htf.Nlist(x, index=idx)
    return htf.compute_nlist_forces(nl, lay(nl, p.to(x.dtype)), virial=virial)


# ------------------------------------------------------------------------------------------------ 1. values
@functools.lru_cache(maxsize=None)
def _case(l_max, K, n_types, activation, cut, config):
    """A layer on a configuration with its fp64 oracle and fp32 twin, shared by the tensor dtypes."""
    import hoomd_tf_amd as htf
    p, L, rc_list, x, idx = _system(config)
    lay = _layer(htf, K=K, n_types=n_types, activation=activation, high=rc_list, r_cut=0.9 * rc_list if cut else None,
                 seed=5 + n_types + 10 * l_max, l_max=l_max)
    ref = oracle(lay, p, L, x, idx)
    twin = oracle(lay, p, L, x, idx, dtype=torch.float32)
    assert ref[0].abs().max().item() > 1e-3
    return lay, ref, twin


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("config", ["a", "b256"])
@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("activation", ["tanh", "linear"])
@pytest.mark.parametrize("n_types", [1, 2])
@pytest.mark.parametrize("l_max", [1, 2])
def test_forces_and_energy(htf, cuda, l_max, n_types, activation, cut, config, dtype):
    """K = 16 with one type, K = 10 with two (D = 60 at l_max = 2; the data has three types, so type-2 particles are in nobody's
    descriptor and their rows have no reverse terms)."""
    p, L, rc_list, x, idx = _system(config)
    lay, ref, twin = _case(l_max, 16 if n_types == 1 else 10, n_types, activation, cut, config)
    f = _run(htf, lay, p, x.to(dtype), idx)
    assert f.dtype == dtype and f.shape == (len(p), 4)
    _assert_values(f, ref, twin)


@pytest.mark.parametrize("K,l_max", [(32, 1), (21, 2)])
def test_widest_inputs(htf, cuda, K, l_max):
    """D = 64 and D = 63: every lane of the wave holds a network input, and the wave's table row fills its LDS region."""
    p, L, rc_list, x, idx = _system("a")
    lay, ref, twin = _case(l_max, K, 1, "tanh", True, "a")
    assert lay.D == K * (1 + l_max) >= 63
    _assert_values(_run(htf, lay, p, x, idx), ref, twin)


# ------------------------------------------------------------------------------------------------ 2. angles matter
def _triplet(cuda, second):
    """Particle 0 with two neighbors at distance 1, (1, 0, 0) and ``second``; rows 1 and 2 see particle 0 only."""
    a, b = torch.tensor([1.0, 0.0, 0.0]), torch.tensor(second)
    x = torch.zeros((3, 2, 4))
    x[0, 0, :3], x[0, 1, :3], x[1, 0, :3], x[2, 0, :3] = a, b, -a, -b
    idx = torch.tensor([[1, 2], [0, -1], [0, -1]], dtype=torch.int32)
    return x.to(cuda), idx.to(cuda)


def test_angles_matter(htf, cuda):
    """Two neighbors at distance 1, at 90 and at 180 degrees: the same distances, so the same G and the same energy for
    l_max = 0; A = |w u_1 + w u_2|^2 is 2 w^2 at 90 degrees and 0 at 180, and the l_max = 1 energies differ.  (The 1e-7 of
    safe_norm moves r by an ulp between (1, 0, 0) and (-1, 0, 0): G agrees to TOL, not to the bit.)"""
    K = 8
    x90, idx = _triplet(cuda, [0.0, 1.0, 0.0])
    x180, _ = _triplet(cuda, [-1.0, 0.0, 0.0])
    lay = _layer(htf, K=K, high=1.8, l_max=1, seed=7)
    d90, d180 = lay.descriptor(x90).double(), lay.descriptor(x180).double()
    assert d90.shape == (3, 2 * K)
    w = torch.exp(-(1.0 - torch.as_tensor(lay.centers.astype(np.float64), device=cuda)) ** 2 / float(lay.gap))
    assert w.max().item() > 0.5
    _close(d90[0, :K], 2.0 * w, "G at 90")
    _close(d180[0, :K], d90[0, :K], "G at 180 against G at 90")
    _close(d90[0, K:] - d180[0, K:], 2.0 * w * w, "A at 90 minus A at 180")
    _close(d180[0, K:], torch.zeros(K, device=cuda), "A at 180", scale=(2.0 * w * w).max().item())
    e90, e180 = lay.total_forces(x90, idx)[0, 3].item(), lay.total_forces(x180, idx)[0, 3].item()
    print("l_max = 1: E(90) %.6g, E(180) %.6g" % (e90, e180))
    assert abs(e90 - e180) > 1e-3
    lay0 = _layer(htf, K=K, high=1.8, l_max=0, seed=7)
    z90, z180 = lay0.total_forces(x90, idx)[0, 3].item(), lay0.total_forces(x180, idx)[0, 3].item()
    print("l_max = 0: E(90) %.6g, E(180) %.6g" % (z90, z180))
    assert abs(z90 - z180) <= TOL * max(1.0, abs(z90))


# ------------------------------------------------------------------------------------------------ 3. momentum
@pytest.mark.parametrize("l_max", [1, 2])
@pytest.mark.parametrize("config", ["a", "b256"])
def test_momentum(htf, cuda, config, l_max):
    """Every row is within TOL max|F| of the gradient, whose rows sum to zero exactly: |sum_i F_i| <= TOL N max|F| at worst."""
    p, L, rc_list, x, idx = _system(config)
    lay = _layer(htf, K=10, n_types=2, high=rc_list, r_cut=0.9 * rc_list, seed=21, l_max=l_max)
    f = _run(htf, lay, p, x, idx)[:, :3].double()
    bound = TOL * len(p) * f.abs().max().item()
    total = f.sum(dim=0).abs().max().item()
    print("sum F %.3g, bound %.3g" % (total, bound))
    assert f.abs().max().item() > 1e-3 and total <= bound


# ------------------------------------------------------------------------------------------------ 4. virial
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("config,cut,l_max", [("a", True, 1), ("a", False, 2), ("b256", True, 2)])
def test_virial(htf, cuda, config, cut, l_max, dtype):
    p, L, rc_list, x, idx = _system(config)
    lay = _layer(htf, K=10, n_types=2, high=rc_list, r_cut=0.9 * rc_list if cut else None, seed=31, l_max=l_max)
    xx = x.to(dtype)
    f, w = _run(htf, lay, p, xx, idx, virial=True)
    assert w.dtype == dtype and w.shape == (len(p), 3, 3)
    F, E, W, xphi, dE_deps = formula(lay, x, idx, p[:, 3].long())
    # the formula is the gradient: the oracle's forces, to the 1e-7 of the reverse terms
    _close(F, oracle(lay, p, L, x, idx)[0], "formula against autograd", tol=5e-6)
    # phi is not along x: W_i has an antisymmetric part, which the six-entry form of the row operator could not hold
    assert (W - W.transpose(1, 2)).abs().max().item() > 10 * TOL * W.abs().max().item()
    _close(f[:, :3], F, "forces")
    _close(w, W, "virial")
    # the trace of the total is the volume derivative of the total energy
    _close(w.double().diagonal(dim1=1, dim2=2).sum().reshape(1), -dE_deps.reshape(1), "trace", scale=xphi.item())
    # without the virial: the same forces, bit for bit
    assert torch.equal(_run(htf, lay, p, xx, idx), f)


# ------------------------------------------------------------------------------------------------ 5. bits
@pytest.mark.parametrize("l_max", [1, 2])
def test_bits(htf, cuda, l_max):
    p, L, rc_list, x, idx = _system("a")
    lay = _layer(htf, K=6, n_types=3, high=rc_list, r_cut=0.9 * rc_list, seed=41, l_max=l_max)
    types = p[:, 3].contiguous()
    a, va = lay.total_forces(x, idx, virial=True, types=types)
    b, vb = lay.total_forces(x, idx, virial=True, types=types)
    assert torch.equal(a, b) and torch.equal(va, vb)
    da, db = lay.descriptor(x), lay.descriptor(x)
    assert da.shape == (len(p), lay.D) and torch.equal(da, db) and da[:, lay.Dr:].abs().max().item() > 0
    assert torch.equal(lay.descriptor(x.double()), da.double())
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


# ------------------------------------------------------------------------------------------------ 6. edges
@pytest.mark.parametrize("l_max", [1, 2])
def test_edges(htf, cuda, l_max):
    """Indices outside [0, B) on live slots drop that slot's reverse terms and nothing else; a float index tensor is taken by
    rint; a row of empty slots has no force and the energy of input 0; a row whose own type is out of range gathers nothing; a
    neighbor type out of range (three types in the data, n_types = 2) empties the slot's own-row terms only."""
    p, L, rc_list, x, idx = _system("a")
    B = len(p)
    lay = _layer(htf, K=10, n_types=2, high=rc_list, seed=51, l_max=l_max)
    x, idx, types = x.clone(), idx.clone(), p[:, 3].clone()
    assert int((x[:, :, 3] == 2).sum()) > 0 and int((types == 2).sum()) > 0   # neighbor and own types out of range exist
    idx[0, 0], idx[1, 0], idx[2, 1], idx[3, 2] = -1, B, B + 5, -7
    x[5] = 0.0            # (its neighbors still read row 5's table: dE/d(input) at input 0, p = S = 0)
    types[7] = 3.0        # out of range whatever it was: row 7 has own-row terms only
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


@pytest.mark.parametrize("NN", [1, 64, 65])
def test_slot_counts(htf, cuda, NN):
    """One slot per row (a list cut short is not symmetric: the formula takes any list), a full first slot register and the
    first slot of the second."""
    p, L, rc_list, x, idx = _system("a")
    if NN < x.shape[1]:
        x, idx = x[:, :NN].contiguous(), idx[:, :NN].contiguous()
    else:
        pad = NN - x.shape[1]
        x = torch.cat([x, torch.zeros((len(p), pad, 4), device=cuda)], dim=1).contiguous()
        idx = torch.cat([idx, torch.full((len(p), pad), -1, dtype=torch.int32, device=cuda)], dim=1).contiguous()
        x[:, -1], idx[:, -1] = x[:, 0].clone(), idx[:, 0].clone()   # the last slot is live: slot 0 moved there
        x[:, 0], idx[:, 0] = 0.0, -1
    lay = _layer(htf, K=10, n_types=2, high=rc_list, r_cut=0.9 * rc_list, seed=55, l_max=2)
    f, w = lay.total_forces(x, idx, virial=True, types=p[:, 3].contiguous())
    F, E, W, _, _ = formula(lay, x, idx, p[:, 3].long())
    assert F.abs().max().item() > 1e-3
    _close(f[:, :3], F, "forces")
    _close(f[:, 3], E, "energy")
    _close(w, W, "virial")


@pytest.mark.parametrize("l_max", [1, 2])
def test_zero_rows(htf, cuda, l_max):
    lay = _layer(htf, K=8, n_types=2, l_max=l_max)
    for dt in (torch.float32, torch.float64):
        x = torch.zeros((0, 32, 4), dtype=dt, device=cuda)
        f, v = lay.total_forces(x, torch.zeros((0, 32), dtype=torch.int32, device=cuda), virial=True,
                                types=torch.zeros((0,), device=cuda))
        assert f.shape == (0, 4) and v.shape == (0, 3, 3) and f.dtype == dt
        d = lay.descriptor(x)
        assert d.shape == (0, lay.D) and d.dtype == dt


# ------------------------------------------------------------------------------------------------ 7. species
@pytest.mark.parametrize("empty", [False, True])
def test_one_network_per_species(htf, cuda, empty):
    """n_species = 2 with l_max = 1; ``empty``: every row is of species 0, network 1 has no rows and no launch."""
    p, L, rc_list, x, idx = _system("a")
    lay = _layer(htf, K=10, n_types=2, high=rc_list, r_cut=0.9 * rc_list, n_species=2, seed=11, l_max=1)
    sp = torch.zeros(len(p), dtype=torch.long, device=cuda) if empty else (p[:, 3].long() % 2)
    f = lay.total_forces(x, idx, types=p[:, 3].contiguous(), species=sp.to(torch.float32))
    _assert_values(f, oracle(lay, p, L, x, idx, sp=sp), oracle(lay, p, L, x, idx, sp=sp, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ 8. l_max = 0 is untouched
def test_l_max_zero_is_the_radial_layer(htf, cuda):
    p, L, rc_list, x, idx = _system("a")
    kw = dict(K=10, H1=32, H2=24, low=0.5, high=rc_list, n_types=3, r_cut=0.9 * rc_list, seed=9, conservative=True)
    a, b = htf.DescriptorMLP(l_max=0, **kw), htf.DescriptorMLP(**kw)
    assert torch.equal(a.w, b.w)
    types = p[:, 3].contiguous()
    fa, va = a.total_forces(x, idx, virial=True, types=types)
    fb, vb = b.total_forces(x, idx, virial=True, types=types)
    assert fb[:, :3].abs().max().item() > 1e-3
    assert torch.equal(fa, fb) and torch.equal(va, vb)
    assert torch.equal(a.descriptor(x), b.descriptor(x)) and torch.equal(a.forces(x), b.forces(x))


# ------------------------------------------------------------------------------------------------ 9. through tfcompute
def _fcc(cuda, seed, types=None):
    from hoomd_tf_amd import standin
    pos, L, a = standin.fcc_positions(5, 0.8442)
    rng = np.random.default_rng(seed)
    pos = pos + 0.03 * a * rng.standard_normal(pos.shape)
    pos -= np.round(pos / L) * L
    return standin.System(pos, L, types=types, dtype=torch.float32, device=cuda), float(L[0])


def _sim(htf, cuda, seed):
    from hoomd_tf_amd import standin
    sysm, L = _fcc(cuda, seed)
    sysm.randomize_velocities(kT=0.3, seed=seed)
    sim = standin.Simulation(sysm)
    sim.integrate_nve(0.001)
    return sim, sysm, L


def _model(htf, lay):
    class M(htf.SimModel):
        def setup(self):
            self.desc = lay
            self.seen = None

        def compute(self, nlist, positions, box):
            self.seen = positions.detach().clone()
            return htf.compute_nlist_forces(nlist, self.desc(nlist, positions))
    return M


def _all_pairs(lay, seen, L, dtype):
    """(F, E) by autograd over every pair under minimum image, no list and no index: valid because fc vanishes before the
    list's cutoff."""
    N = len(seen)
    q = seen[:, :3].to(dtype).requires_grad_(True)
    d = q[None, :, :] - q[:, None, :]
    d = d - L * torch.round(d.detach() / L)
    off = ~torch.eye(N, dtype=torch.bool, device=seen.device)
    X = _inputs(lay, d * off[..., None].to(dtype), torch.zeros((N, N), dtype=torch.float64, device=seen.device))[0]
    E = _network(lay, X, torch.zeros(N, dtype=torch.long, device=seen.device))
    (g,) = torch.autograd.grad(E.sum(), q)
    return -g.detach(), E.detach()


def test_nve_through_tfcompute(htf, cuda):
    """Five NVE steps of 500 particles with l_max = 2, r_cut = 2.0 in a list of 2.5.  The last forces equal the all-pairs fp64
    gradient at the positions they were evaluated at.  Momentum: each step adds dt sum_i F_i, at most dt TOL N max|F|
    (test_momentum), and each of the N fp32 updates v += f dt rounds once, by at most 2^-24 max|v| (half an ulp)."""
    steps, dt = 5, 0.001
    lay = _layer(htf, K=16, high=2.0, r_cut=2.0, seed=71, l_max=2)
    sim, sysm, L = _sim(htf, cuda, 73)
    model = _model(htf, lay)(128)
    tfc = htf.tfcompute(model)
    tfc.attach(sim.nlist_cell(), r_cut=2.5)
    p0 = sysm.vel[:sysm.N, :3].double().sum(dim=0)
    sim.run(steps)
    torch.cuda.synchronize()
    assert tfc._plan is None and not tfc.graph_safe()
    f = sysm.force[:sysm.N].double()
    ref = _all_pairs(lay, model.seen, L, torch.float64)
    assert ref[0].abs().max().item() > 1e-2
    _assert_values(f, ref, _all_pairs(lay, model.seen, L, torch.float32))
    dp = (sysm.vel[:sysm.N, :3].double().sum(dim=0) - p0).abs().max().item()
    vmax, fmax = sysm.vel[:sysm.N, :3].abs().max().item(), ref[0].abs().max().item()
    bound = steps * sysm.N * (2.0 ** -24 * vmax + dt * TOL * fmax)
    print("momentum drift %.3g, bound %.3g" % (dp, bound))
    assert dp <= bound


def test_batches_raise(htf, cuda):
    sim, sysm, _ = _sim(htf, cuda, 83)
    tfc = htf.tfcompute(_model(htf, _layer(htf, K=8, high=2.0, r_cut=2.0, l_max=2))(128))
    tfc.attach(sim.nlist_cell(), r_cut=2.5, batch_size=sysm.N // 3)
    with pytest.raises(ValueError, match="batch"):
        sim.run(1)
