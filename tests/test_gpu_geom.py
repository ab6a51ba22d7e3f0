"""Molecular geometry on the GPU (csrc/mol_geom.hip): ``mol_bond_distance``, ``mol_angle`` and ``mol_dihedral`` against an
fp64 restatement of their definitions on the same fp32 inputs, upstream's acos forms where upstream is right, fp64 autograd
for the gradients, determinism of the CG backward, the cached index tables, and both modes end to end (MolFeatureModel of
hoomd-tf's build_examples.py through tfcompute; a CG energy through center_of_mass to atom forces).

Value tolerance.  The kernel sees the same fp32 coordinates as the restatement; what differs is its fp32 arithmetic.  The
minimum image of p_j - p_i rounds twice at the scale of the box (the difference, then d - rint(d/L) L): each component is
off by at most 2 ulp(L), a vector by 2 sqrt(3) ulp(L).  The vector products after it round at the scale of the vectors,
which amounts to a perturbation of the same order.  So each point is taken as moved by at most DELTA = 8 ulp(L), and a
term may be off by DELTA * sum_k |d value / d p_k| (for a bond or an angle: DELTA over the bond length) plus the rounding
of the final sqrt / atan2, 16 eps32 * max(value, 1)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------------------------------------ restatements
def _geom_t(P, L):
    """fp64 torch restatement on [T, K, 3] points (differentiable): bond, angle (atan2) or |dihedral| (0 where n1 or n2
    vanishes, with a zero gradient there)."""
    K = P.shape[1]

    def mi(d):
        return d - torch.round(d / L).detach() * L

    def norm(v):
        n2 = (v * v).sum(-1)
        ok = n2 > 0
        return torch.where(ok, torch.sqrt(torch.where(ok, n2, torch.ones_like(n2))), torch.zeros_like(n2)), ok

    if K == 2:
        return norm(mi(P[:, 1] - P[:, 0]))[0]
    if K == 3:
        a, b = mi(P[:, 0] - P[:, 1]), mi(P[:, 2] - P[:, 1])
        s, _ = norm(torch.cross(a, b, dim=-1))
        return torch.atan2(s, (a * b).sum(-1))
    b1, b2, b3 = mi(P[:, 1] - P[:, 0]), mi(P[:, 2] - P[:, 1]), mi(P[:, 3] - P[:, 2])
    n1, n2 = torch.cross(b1, b2, dim=-1), torch.cross(b2, b3, dim=-1)
    _, ok1 = norm(n1)
    _, ok2 = norm(n2)
    g, _ = norm(b2)
    ok = ok1 & ok2
    y, x = g * (b1 * n2).sum(-1), (n1 * n2).sum(-1)
    phi = torch.atan2(torch.where(ok, y, torch.zeros_like(y)), torch.where(ok, x, torch.ones_like(x)))
    return torch.where(ok, phi.abs(), torch.zeros_like(phi))


def _ref_and_tol(P32, L, dev):
    """fp64 values of the [T, K, 3] fp32 points and the per-term bound of the module docstring."""
    P = torch.from_numpy(np.asarray(P32, np.float64)).to(dev).requires_grad_(True)
    v = _geom_t(P, L)
    (g,) = torch.autograd.grad(v.sum(), P)
    delta = 8.0 * float(np.spacing(np.float32(L)))
    tol = delta * g.norm(dim=-1).sum(-1) + 16 * EPS32 * torch.clamp(v.detach().abs(), min=1.0)
    return v.detach().cpu().numpy(), tol.cpu().numpy()


def _chains(n_chain, n_per, L, seed, bond=(0.8, 1.2), max_cos=0.9, wrap=True):
    """Random-walk chains in a periodic box of side L, wrapped into [-L/2, L/2) (unless ``wrap`` is False): bond lengths in
    ``bond``, successive bonds at |cos| <= max_cos (no near-collinear triples).  float32 [n_chain, n_per, 3]."""
    rng = np.random.default_rng(seed)
    p = np.zeros((n_chain, n_per, 3))
    p[:, 0] = rng.uniform(-L / 2, L / 2, (n_chain, 3))
    prev = None
    for i in range(1, n_per):
        u = rng.normal(size=(n_chain, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        if prev is not None:
            bad = np.abs((u * prev).sum(1)) > max_cos
            while bad.any():
                v = rng.normal(size=(int(bad.sum()), 3))
                u[bad] = v / np.linalg.norm(v, axis=1, keepdims=True)
                bad = np.abs((u * prev).sum(1)) > max_cos
        p[:, i] = p[:, i - 1] + u * rng.uniform(*bond, (n_chain, 1))
        prev = u
    if wrap:
        p = p - np.round(p / L) * L
    return p.astype(np.float32)


def _chain_terms(n_chain, n_per, K):
    """The K-point terms along every chain of a [n_chain * n_per] bead array: K index arrays."""
    base = (np.arange(n_chain)[:, None] * n_per + np.arange(n_per - K + 1)[None, :]).reshape(-1)
    return [base + s for s in range(K)]


def _with_types(p):
    return np.concatenate([p, np.zeros(p.shape[:-1] + (1,), np.float32)], -1)


OPS = {2: "mol_bond_distance", 3: "mol_angle", 4: "mol_dihedral"}


def _call_mol(htf, K, mol_pos, slots, box):
    return getattr(htf, OPS[K])(mol_pos, *slots, box=box)


def _call_cg(htf, K, cg, idx, box):
    return getattr(htf, OPS[K])(CG=True, cg_positions=cg, box=box, **{"b%d" % (s + 1): idx[s] for s in range(K)})


def _box(L, dev=None):
    b = torch.tensor([[-L / 2] * 3, [L / 2] * 3, [0.0] * 3], dtype=torch.float32)
    return b.to(dev) if dev is not None else b


# ------------------------------------------------------------------------------------------------ 1. values vs fp64
@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("M", [1, 10, 1000, 200000])
def test_mol_mode_values_vs_f64(htf, cuda, K, M):
    L = 6.0
    MN = 6
    p = _chains(M, MN, L, seed=K * 7 + M)
    mol = torch.from_numpy(_with_types(p)).to(cuda)
    for slots in ([0, 1, 2, 3][:K], [5, 4, 3, 2][:K], [1, 3, 4, 5][:K]):
        got = _call_mol(htf, K, mol, slots, _box(L, cuda))
        assert got.shape == (M,) and got.dtype == torch.float32
        ref, tol = _ref_and_tol(p[:, slots], L, cuda)
        err = np.abs(got.cpu().numpy() - ref)
        assert (err <= tol).all(), (err.max(), tol[np.argmax(err - tol)])


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("n_chain", [1, 3, 1000, 7875])
def test_cg_mode_values_vs_f64(htf, cuda, K, n_chain):
    """Chains of 128 beads in a box of side 9: bonds cross every face; up to 1 000 000 terms (7 875 chains)."""
    L, n_per = 9.0, 128
    p = _chains(n_chain, n_per, L, seed=100 + K)
    flat = p.reshape(-1, 3)
    idx = _chain_terms(n_chain, n_per, K)
    T = len(idx[0])
    if n_chain >= 1000:
        raw = flat[idx[1]] - flat[idx[0]]
        for c in range(3):
            assert (raw[:, c] > L / 2).any() and (raw[:, c] < -L / 2).any()   # (crossings of both faces, every axis)
    cg = torch.from_numpy(_with_types(flat)).to(cuda)
    ref, tol = _ref_and_tol(flat[np.stack(idx, 1)], L, cuda)
    for form in ("device", "numpy"):
        ix = [torch.from_numpy(i).to(cuda) for i in idx] if form == "device" else idx
        got = _call_cg(htf, K, cg, ix, _box(L, cuda))
        assert got.shape == (T,)
        err = np.abs(got.cpu().numpy() - ref)
        assert (err <= tol).all(), (form, err.max())
    # the [B, 3] view gives the same bits as the [B, 4] rows read with their stride
    got3 = _call_cg(htf, K, cg[:, :3].contiguous(), idx, _box(L, cuda))
    np.testing.assert_array_equal(got3.cpu().numpy(), got.cpu().numpy())


@pytest.mark.parametrize("K", [2, 3, 4])
def test_cg_scalar_indices(htf, cuda, K):
    L = 7.0
    p = _chains(1, 8, L, seed=K)[0]
    cg = torch.from_numpy(p).to(cuda)
    for start in range(0, 8 - K + 1):
        ids = list(range(start, start + K))[::-1 if start % 2 else 1]
        got = _call_cg(htf, K, cg, ids, _box(L, cuda))
        assert got.dim() == 0
        ref, tol = _ref_and_tol(p[ids][None], L, cuda)
        assert abs(got.item() - ref[0]) <= tol[0]
        np.testing.assert_array_equal(got.cpu().numpy(), _call_cg(htf, K, cg, [np.array([i]) for i in ids],
                                                                  _box(L, cuda)).cpu().numpy()[0])


def test_float64_in_float64_out(htf, cuda):
    L = 6.0
    p = _chains(50, 5, L, seed=3)
    mol = torch.from_numpy(p).double().to(cuda).requires_grad_(True)
    a = htf.mol_angle(mol, 0, 1, 2, box=_box(L, cuda).double())
    assert a.dtype == torch.float64
    (g,) = torch.autograd.grad(a.sum(), mol)
    assert g.dtype == torch.float64 and torch.isfinite(g).all()
    a32 = htf.mol_angle(torch.from_numpy(p).to(cuda), 0, 1, 2, box=_box(L, cuda))
    np.testing.assert_array_equal(a.detach().cpu().numpy(), a32.cpu().numpy().astype(np.float64))


# ------------------------------------------------------------------------------------------------ 2. upstream parity
def _upstream_acos(P, K, per_molecule_norm):
    """hoomd-tf's tensor formulas in fp64 (utils.py mol_angle / mol_dihedral, all-atom branch): acos of normalised dot
    products.  per_molecule_norm=False is upstream's tf.norm(n1) over all molecules."""
    P = np.asarray(P, np.float64)
    if K == 2:
        return np.linalg.norm(P[:, 1] - P[:, 0], axis=1)
    if K == 3:
        a, b = P[:, 0] - P[:, 1], P[:, 2] - P[:, 1]
        return np.arccos((a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)))
    n1 = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 1])
    n2 = np.cross(P[:, 2] - P[:, 1], P[:, 3] - P[:, 2])
    if per_molecule_norm:
        n1 = n1 / np.linalg.norm(n1, axis=1, keepdims=True)
        n2 = n2 / np.linalg.norm(n2, axis=1, keepdims=True)
    else:
        n1, n2 = n1 / np.linalg.norm(n1), n2 / np.linalg.norm(n2)
    return np.arccos((n1 * n2).sum(1))


@pytest.mark.parametrize("K", [2, 3, 4])
def test_one_molecule_equals_upstream(htf, cuda, K):
    """One molecule, no wrapping needed (centred in the box): the three ops equal upstream's acos forms, away from 0 and
    pi, to the bound of the module docstring."""
    L = 8.0
    n = 0
    for seed in range(40):
        p = _chains(1, 4, L, seed=seed, wrap=False)
        p -= p.mean(axis=1, keepdims=True)
        ref = _upstream_acos(p[:, :K], K, per_molecule_norm=False)
        if K > 2 and not 0.05 < ref[0] < math.pi - 0.05:
            continue
        n += 1
        got = _call_mol(htf, K, torch.from_numpy(p).to(cuda), list(range(K)), _box(L, cuda)).cpu().numpy()
        _, tol = _ref_and_tol(p[:, :K], L, cuda)
        assert abs(got[0] - ref[0]) <= tol[0]
    assert n >= 20


def test_several_molecules_dihedral_departs_from_upstream(htf, cuda):
    """Upstream's all-atom dihedral normalises n1 and n2 by their norms over ALL molecules: for M > 1 it is no dihedral.
    The op gives each molecule's own dihedral instead (upstream's value for that molecule alone)."""
    L = 8.0
    p = _chains(16, 4, L, seed=11, wrap=False)
    p -= p.mean(axis=1, keepdims=True)
    got = htf.mol_dihedral(torch.from_numpy(p).to(cuda), 0, 1, 2, 3, box=_box(L, cuda)).cpu().numpy()
    per_term = _upstream_acos(p, 4, per_molecule_norm=True)
    upstream = _upstream_acos(p, 4, per_molecule_norm=False)
    _, tol = _ref_and_tol(p, L, cuda)
    away = (per_term > 0.05) & (per_term < math.pi - 0.05)
    assert away.sum() >= 12
    assert (np.abs(got - per_term)[away] <= tol[away]).all()
    assert np.abs(got - upstream).max() > 0.1                 # (the departure, asserted)
    for m in np.nonzero(away)[0][:3]:
        assert abs(got[m] - _upstream_acos(p[m:m + 1], 4, per_molecule_norm=False)[0]) <= tol[m]


# ------------------------------------------------------------------------------------------------ 3. near-degenerate
def test_angle_near_zero_and_pi(htf, cuda):
    L = 20.0
    for theta in (1e-3, math.pi - 1e-3, 1e-5, math.pi - 1e-5):
        rng = np.random.default_rng(int(theta * 1e6))
        pts = []
        for _ in range(64):
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            w = np.cross(u, rng.normal(size=3))
            w /= np.linalg.norm(w)
            j = rng.uniform(-3, 3, 3)
            r1, r2 = rng.uniform(0.8, 1.5, 2)
            pts.append([j + r1 * u, j, j + r2 * (math.cos(theta) * u + math.sin(theta) * w)])
        P = np.asarray(pts, np.float32)
        got = htf.mol_angle(torch.from_numpy(P).to(cuda), 0, 1, 2, box=_box(L, cuda)).cpu().numpy()
        ref, tol = _ref_and_tol(P, L, cuda)
        assert np.isfinite(got).all()
        err = np.abs(got - ref)
        assert (err <= tol).all(), (theta, err.max(), tol.max())
        # acos of the fp32 cosine cannot resolve these: its error near 0 alone is ~sqrt(2 eps32) = 5e-4
        assert err.max() < 1e-4


def test_degenerate_terms_are_finite_with_zero_gradient(htf, cuda):
    """Lattice points on the x axis: collinear angles (pi and 0), collinear dihedrals, a zero-length bond."""
    L = 10.0
    mol = torch.tensor([[[0.0, 1.0, 1.0], [1.0, 1.0, 1.0], [2.0, 1.0, 1.0], [3.0, 1.0, 1.0]],
                        [[0.0, 1.0, 1.0], [0.0, 1.0, 1.0], [2.0, 1.0, 1.0], [1.0, 1.0, 1.0]]], device=cuda, requires_grad=True)
    box = _box(L, cuda)
    r = htf.mol_bond_distance(mol, 0, 1, box=box)
    a = htf.mol_angle(mol, 0, 1, 2, box=box)
    a2 = htf.mol_angle(mol, 0, 2, 3, box=box)
    d = htf.mol_dihedral(mol, 0, 1, 2, 3, box=box)
    np.testing.assert_array_equal(r.detach().cpu().numpy(), [1.0, 0.0])
    np.testing.assert_allclose(a.detach().cpu().numpy(), [math.pi, 0.0], atol=1e-7)    # (atan2(0, -1), atan2(0, 0))
    np.testing.assert_allclose(a2.detach().cpu().numpy(), [math.pi, 0.0], atol=1e-7)
    np.testing.assert_array_equal(d.detach().cpu().numpy(), [0.0, 0.0])
    for v, zero_rows in ((r, [1]), (a, [0, 1]), (a2, [0, 1]), (d, [0, 1])):
        (g,) = torch.autograd.grad(v.sum(), mol)
        assert torch.isfinite(g).all()
        assert (g[zero_rows] == 0).all()
    # CG mode: the same beads, a bead repeated in a term
    cg = mol.detach()[0]
    for K, ids in ((2, [1, 1]), (3, [0, 1, 2]), (4, [0, 1, 2, 3])):
        x = cg.clone().requires_grad_(True)
        v = _call_cg(htf, K, x, [torch.tensor([i], device=cuda) for i in ids], box)
        (g,) = torch.autograd.grad(v.sum(), x)
        assert torch.isfinite(v).all() and (g == 0).all()


# ------------------------------------------------------------------------------------------------ 4. gradients
@pytest.mark.parametrize("K", [2, 3, 4])
def test_mol_gradients_vs_autograd_f64(htf, cuda, K):
    L = 6.0
    p = _with_types(_chains(500, 6, L, seed=40 + K))
    slots = [4, 2, 1, 0][:K]
    u = torch.from_numpy(np.random.default_rng(K).normal(size=500)).to(cuda)
    x = torch.from_numpy(p).to(cuda).requires_grad_(True)
    (g,) = torch.autograd.grad((_call_mol(htf, K, x, slots, _box(L, cuda)) * u.float()).sum(), x)
    x64 = torch.from_numpy(p).double().to(cuda).requires_grad_(True)
    (g64,) = torch.autograd.grad((_geom_t(x64[:, slots, :3], L) * u).sum(), x64)
    np.testing.assert_allclose(g.cpu().numpy(), g64.cpu().numpy(), rtol=0, atol=1e-4 * g64.abs().max().item())
    assert (g[:, :, 3] == 0).all() and (g[:, [s for s in range(6) if s not in slots]] == 0).all()


@pytest.mark.parametrize("K", [2, 3, 4])
def test_cg_gradients_vs_autograd_f64(htf, cuda, K):
    L, n_chain, n_per = 8.0, 200, 32
    flat = _with_types(_chains(n_chain, n_per, L, seed=50 + K).reshape(-1, 3))
    idx = _chain_terms(n_chain, n_per, K)
    u = torch.from_numpy(np.random.default_rng(K).normal(size=len(idx[0]))).to(cuda)
    x = torch.from_numpy(flat).to(cuda).requires_grad_(True)
    (g,) = torch.autograd.grad((_call_cg(htf, K, x, [torch.from_numpy(i).to(cuda) for i in idx], _box(L, cuda))
                                * u.float()).sum(), x)
    x64 = torch.from_numpy(flat).double().to(cuda).requires_grad_(True)
    P = torch.stack([x64[torch.from_numpy(i).to(cuda), :3] for i in idx], 1)
    (g64,) = torch.autograd.grad((_geom_t(P, L) * u).sum(), x64)
    np.testing.assert_allclose(g.cpu().numpy(), g64.cpu().numpy(), rtol=0, atol=1e-4 * g64.abs().max().item())


@pytest.mark.parametrize("K", [2, 3, 4])
def test_finite_difference_f32(htf, cuda, K):
    """Central differences in fp32 (h = 1e-2) on two molecules, tolerance 5e-3 of the largest gradient entry: truncation
    O(h^2) with third derivatives of order 1/(r sin)^3 <= ~10 here, rounding ~1e-6 / h."""
    L = 7.0
    p = _chains(2, 4, L, seed=60 + K)
    f = lambda q: _call_mol(htf, K, q, list(range(K)), _box(L, cuda)).sum()   # noqa: E731
    x = torch.from_numpy(p).to(cuda).requires_grad_(True)
    (g,) = torch.autograd.grad(f(x), x)
    h = 1e-2
    fd = np.zeros_like(p)
    for idx in np.ndindex(*p.shape):
        xp, xm = p.copy(), p.copy()
        xp[idx] += h
        xm[idx] -= h
        fd[idx] = (f(torch.from_numpy(xp).to(cuda)).item() - f(torch.from_numpy(xm).to(cuda)).item()) / (2 * h)
    g = g.cpu().numpy()
    assert np.abs(g - fd).max() <= 5e-3 * max(np.abs(g).max(), 1.0)


# ------------------------------------------------------------------------------------------------ 5. determinism
@pytest.mark.parametrize("K", [2, 3, 4])
def test_cg_backward_is_bitwise_reproducible(htf, cuda, K):
    """Beads in up to K terms of each kind (chains), plus every term three times over (a bead in 3K terms): two backward
    calls are bitwise identical and equal the fp64 sum of the same contributions."""
    L, n_chain, n_per = 8.0, 2000, 64
    flat = _chains(n_chain, n_per, L, seed=70 + K).reshape(-1, 3)
    idx = [np.concatenate([i, i, i]) for i in _chain_terms(n_chain, n_per, K)]
    ix = [torch.from_numpy(i).to(cuda) for i in idx]
    u = torch.from_numpy(np.random.default_rng(K).normal(size=len(idx[0])).astype(np.float32)).to(cuda)
    x = torch.from_numpy(flat).to(cuda).requires_grad_(True)
    v = _call_cg(htf, K, x, ix, _box(L, cuda))
    (g1,) = torch.autograd.grad(v, x, u, retain_graph=True)
    (g2,) = torch.autograd.grad(v, x, u)
    assert torch.equal(g1, g2)
    x64 = torch.from_numpy(flat).double().to(cuda).requires_grad_(True)
    P = torch.stack([x64[j] for j in ix], 1)
    (g64,) = torch.autograd.grad((_geom_t(P, L) * u.double()).sum(), x64)
    np.testing.assert_allclose(g1.cpu().numpy(), g64.cpu().numpy(), rtol=0, atol=1e-4 * g64.abs().max().item())


# ------------------------------------------------------------------------------------------------ 6. the cache
def test_cg_table_cache_follows_writes(htf, cuda):
    from hoomd_tf_amd import molgeom
    L = 8.0
    flat = _chains(4, 16, L, seed=80).reshape(-1, 3)
    x = torch.from_numpy(flat).to(cuda)
    b1 = torch.arange(0, 63, device=cuda)
    b2 = torch.arange(1, 64, device=cuda)
    t1 = molgeom._device_table((b1, b2), 64, cuda, 2)
    assert molgeom._device_table((b1, b2), 64, cuda, 2) is t1          # (a hit: nothing rebuilt)
    a = htf.mol_bond_distance(CG=True, cg_positions=x, b1=b1, b2=b2, box=_box(L, cuda)).cpu().numpy()
    b2.copy_(torch.flip(b2, [0]))                                     # written in place
    assert molgeom._device_table((b1, b2), 64, cuda, 2) is not t1
    b = htf.mol_bond_distance(CG=True, cg_positions=x, b1=b1, b2=b2, box=_box(L, cuda)).cpu().numpy()
    ref, tol = _ref_and_tol(flat[np.stack([b1.cpu().numpy(), b2.cpu().numpy()], 1)], L, cuda)
    assert (np.abs(b - ref) <= tol).all()
    assert np.abs(a - b).max() > 1.0
    # the range check runs when a table is built: a write out of range is caught at the next call
    b2[0] = 64
    with pytest.raises(ValueError):
        htf.mol_bond_distance(CG=True, cg_positions=x, b1=b1, b2=b2, box=_box(L, cuda))


# ------------------------------------------------------------------------------------------------ 7. molecule mode end to end
def _chain_box(htf, cuda, n_chain=40, n_per=6, L=8.0, seed=90):
    """A stand-in box of bonded chains (system.bonds; find_molecules gives one molecule per chain)."""
    from hoomd_tf_amd import standin
    p = _chains(n_chain, n_per, L, seed=seed, bond=(1.0, 1.1), max_cos=0.7).reshape(-1, 3).astype(np.float64)
    system = standin.System(p, [L] * 3, dtype=torch.float32, device=cuda)
    system.bonds = [(c * n_per + i, c * n_per + i + 1) for c in range(n_chain) for i in range(n_per - 1)]
    return system


def _mol_gather(pos, mol_indices, MN):
    """MolSimModel's mol_positions, restated: a zero row in front, rows by the (+1-shifted, 0-padded) indices."""
    ap = torch.cat([torch.zeros((1, pos.shape[1]), dtype=pos.dtype, device=pos.device), pos], 0)
    return ap[torch.as_tensor(mol_indices, device=pos.device).reshape(-1)].reshape(-1, MN, pos.shape[1])


def test_mol_feature_model_through_tfcompute(htf, cuda):
    from hoomd_tf_amd import standin

    class MolFeatureModel(htf.MolSimModel):
        # build_examples.py:138-147 of hoomd-tf
        def mol_compute(self, nlist, positions, mol_nlist, mol_pos, box):
            r = htf.mol_bond_distance(mol_pos, 2, 1, box=box)
            a = htf.mol_angle(mol_pos, 1, 2, 3, box=box)
            d = htf.mol_dihedral(mol_pos, 1, 2, 3, 4, box=box)
            self.last = (mol_pos.detach().clone().as_subclass(torch.Tensor), r.detach(), a.detach(), d.detach())
            return torch.mean(r), torch.mean(a), torch.mean(d)

    system = _chain_box(htf, cuda)
    L = 8.0
    sim = standin.Simulation(system)
    mol_indices = htf.find_molecules(system)
    assert len(mol_indices) == 40
    MN = 8
    model = MolFeatureModel(MN, [list(m) for m in mol_indices], 16, output_forces=False)
    sim.integrate_nve(0.001).randomize_velocities(kT=0.2, seed=4)
    tfc = htf.tfcompute(model)
    tfc.attach(sim.nlist_cell(), r_cut=2.0, save_output_period=1)
    sim.run(4)
    assert not tfc.graph_safe()
    mol_pos, r, a, d = (t.cpu().numpy() for t in model.last)
    assert mol_pos.shape == (40, MN, 4)
    for K, slots, got in ((2, [2, 1], r), (3, [1, 2, 3], a), (4, [1, 2, 3, 4], d)):
        ref, tol = _ref_and_tol(mol_pos[:, slots, :3], L, cuda)
        assert (np.abs(got - ref) <= tol).all()
    assert len(tfc.outputs) == 3
    np.testing.assert_allclose(np.asarray(tfc.outputs[1]).reshape(-1)[-1], a.mean(), rtol=1e-6)


def test_bonded_energy_forces_through_tfcompute(htf, cuda):
    """Harmonic bond + harmonic angle + cos(phi) dihedral over every molecule, forces by compute_positions_forces, against
    fp64 autograd of the restatement on the positions the model saw.  Stays eager.  (A neighbor-list model's positions
    carry no gradient, so the model gathers its molecules from a differentiable copy through MolSimModel's own index.)"""
    from hoomd_tf_amd import standin
    KB, R0, KA, A0, KD = 50.0, 1.05, 10.0, 1.9, 2.0

    def energy(r, a, d):
        return sum((KB * (v - R0) ** 2).sum() for v in r) + sum((KA * (v - A0) ** 2).sum() for v in a) + \
            sum((KD * torch.cos(v)).sum() for v in d)

    class Bonded(htf.MolSimModel):
        def mol_compute(self, nlist, positions, mol_nlist, mol_pos, box):
            positions = positions.detach().as_subclass(torch.Tensor).requires_grad_(True)
            ap = torch.cat([torch.zeros((1, 4), dtype=positions.dtype, device=positions.device), positions], 0)
            mol_pos = ap.index_select(0, self._mol_flat).reshape(-1, self.MN, 4)
            e = energy([htf.mol_bond_distance(mol_pos, s, s + 1, box=box) for s in range(5)],
                       [htf.mol_angle(mol_pos, s, s + 1, s + 2, box=box) for s in range(4)],
                       [htf.mol_dihedral(mol_pos, s, s + 1, s + 2, s + 3, box=box) for s in range(3)])
            f = htf.compute_positions_forces(positions, e)
            self.last = (positions.detach().clone().as_subclass(torch.Tensor), f.detach().clone())
            return f

    system = _chain_box(htf, cuda, seed=91)
    L = 8.0
    sim = standin.Simulation(system)
    mol_indices = htf.find_molecules(system)
    model = Bonded(6, [list(m) for m in mol_indices], 16)
    sim.integrate_nve(0.0005).randomize_velocities(kT=0.1, seed=5)
    tfc = htf.tfcompute(model)
    tfc.attach(sim.nlist_cell(), r_cut=2.0)
    sim.run(5)
    assert not tfc.graph_safe()
    pos, F = model.last
    x64 = pos.double().requires_grad_(True)
    shifted = [[i + 1 for i in m] for m in mol_indices]
    mp = _mol_gather(x64, shifted, 6)[:, :, :3]
    e = energy([_geom_t(mp[:, [s, s + 1]], L) for s in range(5)],
               [_geom_t(mp[:, [s, s + 1, s + 2]], L) for s in range(4)],
               [_geom_t(mp[:, [s, s + 1, s + 2, s + 3]], L) for s in range(3)])
    (g64,) = torch.autograd.grad(e, x64)
    F64 = -g64[:, :3].cpu().numpy()
    F = F[:, :3].cpu().numpy()
    assert np.abs(F64).max() > 1.0
    assert np.abs(F - F64).max() <= 2e-4 * np.abs(F64).max()
    np.testing.assert_allclose(system.force[:system.N, :3].cpu().numpy(), F, rtol=0, atol=1e-6 * np.abs(F).max())


# ------------------------------------------------------------------------------------------------ 8. CG mode end to end
def test_cg_energy_forces_through_center_of_mass(htf, cuda):
    """Twelve-atom chains mapped 3:1 onto four beads (mass-weighted): center_of_mass -> bond / angle / dihedral of the
    beads (CG=True, device index tensors) -> energy -> atom forces, against fp64 autograd through the dense mapping."""
    from hoomd_tf_amd import standin
    n_side, a = 6, 1.6
    rng = np.random.default_rng(17)
    g = np.stack(np.meshgrid(*[np.arange(n_side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    L = n_side * a
    pos = g * a - L / 2 + 0.25 * a + rng.normal(0, 0.15, g.shape)
    N = pos.shape[0]
    system = standin.System(pos, [L] * 3, dtype=torch.float32, device=cuda)
    system.bonds = [(m * 12 + i, m * 12 + i + 1) for m in range(N // 12) for i in range(11)]
    system.vel[:, 3] = torch.from_numpy(np.tile([12.0, 1.0, 16.0], N // 3).astype(np.float32)).to(cuda)
    index = htf.find_molecules(system)
    assert len(index) == N // 12
    mm = np.repeat(np.eye(4, dtype=np.int32), 3, axis=1)
    s = htf.sparse_mapping([mm for _ in index], index, system=system)
    n_mol = len(index)
    terms = {K: [torch.from_numpy(i).to(cuda) for i in _chain_terms(n_mol, 4, K)] for K in (2, 3, 4)}
    box = _box(L, cuda)

    def energy(r, ang, d):
        return (5.0 * (r - 1.5) ** 2).sum() + (2.0 * (ang - 2.0) ** 2).sum() + torch.cos(d).sum()

    x = system.pos[:system.N, :3].detach().clone().requires_grad_(True)
    com = htf.center_of_mass(x, s, [L] * 3)
    e = energy(_call_cg(htf, 2, com, terms[2], box), _call_cg(htf, 3, com, terms[3], box), _call_cg(htf, 4, com, terms[4], box))
    F = htf.compute_positions_forces(x, e)[:, :3].cpu().numpy()
    x64 = x.detach().double().requires_grad_(True)
    dense = s.to_dense().double()
    theta = x64 / L * 2 * math.pi
    c64 = torch.atan2(dense @ torch.sin(theta), dense @ torch.cos(theta)) * L / (2 * math.pi)
    P = {K: torch.stack([c64[i] for i in terms[K]], 1) for K in (2, 3, 4)}
    e64 = energy(_geom_t(P[2], L), _geom_t(P[3], L), _geom_t(P[4], L))
    (g64,) = torch.autograd.grad(e64, x64)
    F64 = -g64.cpu().numpy()
    assert np.abs(F64).max() > 0.1
    assert np.abs(F - F64).max() <= 2e-4 * np.abs(F64).max()


# ------------------------------------------------------------------------------------------------ 9. validation
def test_validation_on_device(htf, cuda):
    box = _box(10.0, cuda)
    cg = torch.zeros((6, 4), device=cuda)
    mol = torch.zeros((3, 5, 4), device=cuda)
    bad = [
        lambda: htf.mol_bond_distance(mol, 0, 5, box=box),                                  # slot out of range
        lambda: htf.mol_angle(mol, 0, 1, 1, box=box),                                       # repeated slot
        lambda: htf.mol_angle(mol[0], 0, 1, 2, box=box),                                    # rank
        lambda: htf.mol_angle(mol, 0, 1, 2, box=None),                                      # no box
        lambda: htf.mol_bond_distance(CG=True, cg_positions=cg, b1=torch.tensor([0, 1], device=cuda),
                                      b2=torch.tensor([1, 6], device=cuda), box=box),      # index out of range (device)
        lambda: htf.mol_bond_distance(CG=True, cg_positions=cg, b1=torch.tensor([-1], device=cuda),
                                      b2=torch.tensor([1], device=cuda), box=box),
        lambda: htf.mol_bond_distance(CG=True, cg_positions=cg, b1=[0, 5], b2=[1, 7], box=box),   # (host)
        lambda: htf.mol_angle(CG=True, cg_positions=cg, b1=torch.tensor([0, 1], device=cuda),
                              b2=torch.tensor([1, 2], device=cuda), b3=torch.tensor([2], device=cuda), box=box),  # lengths
        lambda: htf.mol_angle(CG=True, cg_positions=cg, b1=torch.tensor([0], device=cuda), b2=[1], b3=[2], box=box),
        lambda: htf.mol_angle(CG=True, cg_positions=cg, b1=0, b2=[1], b3=[2], box=box),    # mixing ints and arrays
        lambda: htf.mol_bond_distance(CG=True, cg_positions=cg, b1=torch.tensor([0.0], device=cuda),
                                      b2=torch.tensor([1.0], device=cuda), box=box),       # float indices
        lambda: htf.mol_bond_distance(CG=True, cg_positions=cg.cpu(), b1=0, b2=1, box=box),      # CPU positions
        lambda: htf.mol_bond_distance(CG=True, cg_positions=cg.cpu().numpy(), b1=0, b2=1, box=box),
        lambda: htf.mol_bond_distance(CG=True, cg_positions=cg.half(), b1=0, b2=1, box=box),     # dtype
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
    # empty index arrays: an empty result, zero gradients
    x = cg.clone().requires_grad_(True)
    v = htf.mol_dihedral(CG=True, cg_positions=x, b1=[], b2=[], b3=[], b4=[], box=box)
    assert v.shape == (0,)
    (g,) = torch.autograd.grad(v.sum(), x, allow_unused=True)
    assert g is None or (g == 0).all()
