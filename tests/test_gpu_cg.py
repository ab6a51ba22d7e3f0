"""Coarse-grained mapping on the GPU (csrc/cg_map.hip): ``center_of_mass`` and ``compute_nlist`` against the reference's
known answers (test_utils.py:187-270 of hoomd-tf), the numpy oracle, an fp64 restatement, torch autograd in fp64, and
example 02 ("Preparing Coarse-grained Mapped Simulation") run through tfcompute."""
import math

import numpy as np
import pytest
import torch

from oracle import htf_oracle as O

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ restatements
def _nlist_ref(p, r_cut, NN, L, sorted=False, return_types=False, excl=None, rows=None):
    """oracle.compute_nlist row by row (same fp32 arithmetic and stable order), with the reference's exclusion matrix and
    only ``rows`` if given: what the oracle computes, at sizes whose [M, M, 3] it could not hold."""
    p = np.asarray(p, np.float32)
    M = p.shape[0]
    rows = np.arange(M) if rows is None else np.asarray(rows)
    box = np.asarray(L, np.float32).reshape(1, 3)
    k = min(NN, M)
    out = np.zeros((len(rows), NN, 4), np.float32)
    for r, i in enumerate(rows):
        dm = p[:, :3] - p[i, :3][None, :]
        dm = dm - np.round(dm / box) * box
        dist = np.sqrt(np.sum(dm * dm, axis=1))
        mask = (dist <= r_cut) & (dist >= 5e-4)
        if excl is not None:
            mask &= ~excl[i, :] & ~excl[:, i]
        mc = mask.astype(np.float32)
        key = -(dist * mc + (1 - mc) * np.float32(1e20)) if sorted else dist * mc
        idx = np.argsort(-key, kind="stable")[:k]
        w = p[idx, 3] if return_types else idx.astype(np.float32)
        out[r, :k] = np.concatenate([dm[idx], w[:, None]], axis=1) * mc[idx][:, None]
    return out


def _bits(a):
    return (np.asarray(a, np.float32) + np.float32(0.0)).view(np.int32)   # (+0.0: -0.0 and 0.0 are the same empty slot)


def _com_f64(pos, dense_map, L):
    theta = np.asarray(pos, np.float64)[:, :3] / L * 2 * np.pi
    X, Z = dense_map @ np.cos(theta), dense_map @ np.sin(theta)
    return np.arctan2(Z, X) / (2 * np.pi) * L


def _periodic_err(a, b, L):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return np.abs(d - np.round(d / L) * L)


def _chain_mapping(htf, n_mol, atoms, beads, device, masses=None, system=None):
    """``n_mol`` molecules of ``atoms`` consecutive atoms, ``beads`` beads each (atoms split into contiguous runs)."""
    mm = np.zeros((beads, atoms), np.int32)
    for a in range(atoms):
        mm[a * beads // atoms, a] = 1
    index = [list(range(m * atoms, (m + 1) * atoms)) for m in range(n_mol)]
    return htf.sparse_mapping([mm for _ in index], index, system=system, device=device), mm


# ------------------------------------------------------------------------------------------------ 1. reference KATs
def _diag(cuda, N=10, types=False):
    p = torch.arange(N, dtype=torch.float32, device=cuda)[:, None].repeat(1, 3)
    return torch.cat([p, torch.zeros((N, 1), device=cuda)], 1) if types else p


def test_compute_nlist_kats(htf, cuda):
    box = [100.0, 100.0, 100.0]
    nl = htf.compute_nlist(_diag(cuda), 100.0, 9, box, return_types=False, sorted=True).cpu().numpy()
    np.testing.assert_array_almost_equal(nl[0, 0], [1, 1, 1, 1])
    np.testing.assert_array_almost_equal(nl[-1, -1], [-9, -9, -9, 0])
    nl = htf.compute_nlist(_diag(cuda, types=True), 100.0, 9, box, return_types=True, sorted=True).cpu().numpy()
    np.testing.assert_array_almost_equal(nl[0, 0], [1, 1, 1, 0])
    em = np.zeros((10, 10), dtype=bool)
    em[0, 1] = em[0, 2] = True
    nl = htf.compute_nlist(_diag(cuda), 100.0, 9, box, sorted=True, exclusion_matrix=em).cpu().numpy()
    assert nl[0, 0, 3] == 3
    np.testing.assert_array_almost_equal(nl[-1, -1], [-9, -9, -9, 0])
    assert nl[1, 0, 3] == 2      # (symmetric: 1 does not see 0 either)
    nl = htf.compute_nlist(_diag(cuda), 5.5, 9, box, sorted=True).cpu().numpy()
    np.testing.assert_array_almost_equal(nl[0, 0], [1, 1, 1, 1])
    np.testing.assert_array_almost_equal(nl[-1, -1], [0, 0, 0, 0])
    assert nl.dtype == np.float32 and nl.shape == (10, 9, 4)


def test_compute_nlist_validation(htf, cuda):
    box = [10.0, 10.0, 10.0]
    with pytest.raises(ValueError):
        htf.compute_nlist(_diag(cuda), 2.0, 4, box, return_types=True)     # [M, 3] has no types
    with pytest.raises(ValueError):
        htf.compute_nlist(_diag(cuda), 2.0, 257, box)
    with pytest.raises(ValueError):
        htf.compute_nlist(_diag(cuda), 2.0, 0, box)
    with pytest.raises(ValueError):
        htf.compute_nlist(torch.zeros((0, 3), device=cuda), 2.0, 4, box)
    with pytest.raises(ValueError):
        htf.compute_nlist(_diag(cuda), 2.0, 4, box, exclusion_matrix=np.zeros((3, 3), bool))


# ------------------------------------------------------------------------------------------------ 2. vs the oracle
def _cloud(M, seed, L=12.0):
    """Half the particles in a dense corner cluster (rows with far more than NN neighbors), half spread over the box
    (rows with few), some on a lattice of exactly representable points (exact distance ties: i +- v), types 0..3."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-L / 2, L / 2, (M, 3))
    n_dense = M // 2
    p[:n_dense] = rng.uniform(L / 2 - 1.5, L / 2, (n_dense, 3))          # straddles the +x/+y/+z faces
    n_lat = min(M // 4, 64)
    if n_lat:
        g = rng.integers(-8, 8, (n_lat, 3)) * 0.25                       # exact in fp32, so are their differences
        p[M - n_lat:] = g
    t = rng.integers(0, 4, M).astype(np.float32)
    p = np.concatenate([p.astype(np.float32), t[:, None]], 1)
    p[:, :3] -= np.round(p[:, :3] / np.float32(L)).astype(np.float32) * np.float32(L)
    return p.astype(np.float32), L


CASES = [(M, NN, s) for M in (1, 63, 64, 65, 1000) for NN in (1, 16, 64, 256) for s in (True, False)]


@pytest.mark.parametrize("M,NN,sorted_", CASES)
def test_compute_nlist_vs_oracle(htf, cuda, M, NN, sorted_):
    p, L = _cloud(M, seed=M * 7 + NN)
    r_cut = 2.0
    types = (M + NN) % 2 == 1
    x = torch.from_numpy(p if types else p[:, :3].copy()).to(cuda)
    got = htf.compute_nlist(x, r_cut, NN, [L] * 3, sorted=sorted_, return_types=types).cpu().numpy()
    ref = O.compute_nlist(p if types else p[:, :3], r_cut, NN, [L] * 3, sorted=sorted_, return_types=types)
    assert got.shape == (M, NN, 4)
    k = ref.shape[1]
    np.testing.assert_array_equal(got[:, :k, 3], ref[:, :, 3])
    np.testing.assert_array_equal(_bits(got[:, :k, :3]), _bits(ref[:, :, :3]))
    assert not np.any(got[:, k:])
    # the restatement the larger cases use is the oracle here
    np.testing.assert_array_equal(_bits(_nlist_ref(p, r_cut, NN, [L] * 3, sorted_, types)[:, :k]), _bits(ref))
    if M == 1000:
        n = (np.abs(got[:, :, :3]).sum(2) > 0).sum(1)
        assert n.min() < NN or NN == 1
        if NN <= 64:
            assert n.max() == NN         # rows with more candidates than slots


@pytest.mark.parametrize("sorted_,types", [(True, False), (False, True)])
def test_compute_nlist_exclusions_vs_oracle(htf, cuda, sorted_, types):
    M, NN = 1000, 64
    p, L = _cloud(M, seed=11)
    rng = np.random.default_rng(3)
    em = rng.random((M, M)) < 0.2          # not symmetric: the op applies it both ways
    x = torch.from_numpy(p if types else p[:, :3].copy()).to(cuda)
    got = htf.compute_nlist(x, 2.0, NN, [L] * 3, sorted=sorted_, return_types=types,
                            exclusion_matrix=torch.from_numpy(em).to(cuda)).cpu().numpy()
    ref = _nlist_ref(p, 2.0, NN, [L] * 3, sorted_, types, excl=em)
    np.testing.assert_array_equal(got[:, :, 3], ref[:, :, 3])
    np.testing.assert_array_equal(_bits(got[:, :, :3]), _bits(ref[:, :, :3]))
    plain = htf.compute_nlist(x, 2.0, NN, [L] * 3, sorted=sorted_, return_types=types).cpu().numpy()
    assert np.any(plain != got)


@pytest.mark.parametrize("NN,sorted_", [(64, True), (256, False), (256, True)])
def test_compute_nlist_large_vs_restatement(htf, cuda, NN, sorted_):
    M = 20000
    p, L = _cloud(M, seed=NN + sorted_, L=40.0)
    x = torch.from_numpy(p).to(cuda)
    got = htf.compute_nlist(x, 3.0, NN, [L] * 3, sorted=sorted_, return_types=False).cpu().numpy()
    rows = np.concatenate([np.arange(0, M, 97), [M - 1]])
    ref = _nlist_ref(p, 3.0, NN, [L] * 3, sorted_, False, rows=rows)
    np.testing.assert_array_equal(got[rows, :, 3], ref[:, :, 3])
    np.testing.assert_array_equal(_bits(got[rows, :, :3]), _bits(ref[:, :, :3]))


# ------------------------------------------------------------------------------------------------ 3. centre of mass
def _straddling(n_mol, atoms, L, seed, spread=1.0):
    """Molecules centred on every face, edge and corner of the box (and some inside), atoms wrapped into the box."""
    rng = np.random.default_rng(seed)
    anchors = np.array([[a, b, c] for a in (-0.5, 0.0, 0.5) for b in (-0.5, 0.0, 0.5) for c in (-0.5, 0.0, 0.5)]) * L
    centres = anchors[np.arange(n_mol) % len(anchors)] + rng.normal(0, 0.1, (n_mol, 3))
    pos = np.repeat(centres, atoms, axis=0) + rng.uniform(-spread, spread, (n_mol * atoms, 3))
    pos -= np.round(pos / L) * L
    return pos.astype(np.float32)


@pytest.mark.parametrize("n_mol,atoms,beads,weighted", [(54, 6, 2, False), (54, 6, 2, True), (40, 3, 3, False),
                                                        (81, 9, 2, True)])
def test_center_of_mass_vs_f64(htf, cuda, n_mol, atoms, beads, weighted):
    from hoomd_tf_amd import standin
    L = 20.0
    pos = _straddling(n_mol, atoms, L, seed=n_mol + beads)
    N = pos.shape[0]
    system = None
    if weighted:
        system = standin.System(pos, [L] * 3, dtype=torch.float32, device=cuda)
        system.vel[:, 3] = torch.from_numpy(np.random.default_rng(2).uniform(1.0, 16.0, N).astype(np.float32)).to(cuda)
    s, mm = _chain_mapping(htf, n_mol, atoms, beads, cuda, system=system)
    x = torch.from_numpy(pos).to(cuda)
    com = htf.center_of_mass(x, s, [L] * 3).cpu().numpy()
    assert com.shape == (n_mol * beads, 3) and com.dtype == np.float32
    assert np.all(com <= L / 2) and np.all(com > -L / 2)
    ref = _com_f64(pos, s.cpu().to_dense().double().numpy(), L)
    assert _periodic_err(com, ref, L).max() <= 2e-6 * L
    # the same op, called again, from the cached device copies (and a [:, :3] view of an [N, 4] array, a device box)
    x4 = torch.cat([x, torch.ones((N, 1), device=cuda)], 1)
    np.testing.assert_array_equal(htf.center_of_mass(x4[:, :3], s, torch.tensor([L] * 3, device=cuda)).cpu().numpy(), com)


def test_center_of_mass_131072_atoms(htf, cuda):
    """131 072 atoms, 3:1 (the last bead has two), molecules straddling every face and corner, mass-weighted."""
    from hoomd_tf_amd import standin
    N, L = 131072, 110.0
    rng = np.random.default_rng(9)
    pos = _straddling(N // 3 + 1, 3, L, seed=4)[:N]              # (molecules of three: one bead each)
    masses = rng.uniform(1.0, 16.0, N).astype(np.float32)
    system = standin.System(pos, [L] * 3, dtype=torch.float32, device=cuda)
    system.vel[:, 3] = torch.from_numpy(masses).to(cuda)
    index = [list(range(a, min(a + 3, N))) for a in range(0, N, 3)]
    mms = [np.ones((1, len(ix)), np.int32) for ix in index]
    s = htf.sparse_mapping(mms, index, system=system)
    assert tuple(s.shape) == (43691, N)
    com = htf.center_of_mass(torch.from_numpy(pos).to(cuda), s, [L] * 3).cpu().numpy()
    # fp64 restatement, bead by bead of 3 (the last of 2)
    theta = pos.astype(np.float64) / L * 2 * np.pi
    w = masses.astype(np.float64)
    bead = np.arange(N) // 3
    wsum = np.bincount(bead, weights=w)
    X = np.stack([np.bincount(bead, weights=w * np.cos(theta[:, c])) for c in range(3)], 1) / wsum[:, None]
    Z = np.stack([np.bincount(bead, weights=w * np.sin(theta[:, c])) for c in range(3)], 1) / wsum[:, None]
    ref = np.arctan2(Z, X) / (2 * np.pi) * L
    assert _periodic_err(com, ref, L).max() <= 2e-6 * L


def test_center_of_mass_single_atom_beads(htf, cuda):
    """A bead of one atom is that atom (wrapped into (-L/2, L/2])."""
    L = 8.0
    pos = _straddling(27, 1, L, seed=1, spread=0.0)
    s, _ = _chain_mapping(htf, 27, 1, 1, cuda)
    com = htf.center_of_mass(torch.from_numpy(pos).to(cuda), s, [L] * 3).cpu().numpy()
    assert _periodic_err(com, pos, L).max() <= 2e-6 * L


def test_center_of_mass_refuses_sorting(htf, cuda):
    """test_com: with particle sorting on, center_of_mass raises; with it off it runs."""
    from hoomd_tf_amd import standin
    pos = _straddling(4, 10, 10.0, seed=2)
    system = standin.System(pos, [10.0] * 3, dtype=torch.float32, device=cuda)
    sim = standin.Simulation(system)
    nl = sim.nlist_cell()
    s, _ = _chain_mapping(htf, 4, 10, 3, cuda, system=system)
    x = torch.from_numpy(pos).to(cuda)
    nl.sort_particles = True
    with pytest.raises(ValueError):
        htf.center_of_mass(x, s, [10.0] * 3)
    nl.sort_particles = False
    assert htf.center_of_mass(x, s, [10.0] * 3).shape == (12, 3)


def test_center_of_mass_cache_follows_writes(htf, cuda):
    """The device copies are rebuilt when the mapping tensor is written in place (its _version moves)."""
    L = 10.0
    pos = _straddling(6, 4, L, seed=3)
    s, _ = _chain_mapping(htf, 6, 4, 2, cuda)
    x = torch.from_numpy(pos).to(cuda)
    a = htf.center_of_mass(x, s, [L] * 3).cpu().numpy()
    v = s._values()
    v[::2] *= 3.0
    assert s._version != 0 or v._version != 0
    b = htf.center_of_mass(x, s, [L] * 3).cpu().numpy()
    ref = _com_f64(pos, s.cpu().to_dense().double().numpy(), L)
    assert _periodic_err(b, ref, L).max() <= 2e-6 * L
    assert np.abs(a - b).max() > 1e-3


# ------------------------------------------------------------------------------------------------ 4. gradients
def _torch_com(pos64, dense64, L):
    theta = pos64 / L * 2 * math.pi
    return torch.atan2(dense64 @ torch.sin(theta), dense64 @ torch.cos(theta)) * L / (2 * math.pi)


def test_com_backward_vs_autograd_f64(htf, cuda):
    L = 12.0
    pos = _straddling(30, 5, L, seed=6)
    s, _ = _chain_mapping(htf, 30, 5, 2, cuda)
    u = torch.from_numpy(np.random.default_rng(1).normal(size=(60, 3))).to(cuda)
    x = torch.from_numpy(pos).to(cuda).requires_grad_(True)
    (g,) = torch.autograd.grad((htf.center_of_mass(x, s, [L] * 3) * u.float()).sum(), x)
    x64 = torch.from_numpy(pos).double().to(cuda).requires_grad_(True)
    (g64,) = torch.autograd.grad((_torch_com(x64, s.to_dense().double(), L) * u).sum(), x64)
    np.testing.assert_allclose(g.cpu().numpy(), g64.cpu().numpy(), atol=2e-5 * g64.abs().max().item())


def test_com_finite_difference_f32(htf, cuda):
    """The kernels are fp32 only (no fp64 gradcheck): central differences in fp32, h = 1e-2, tolerance 2e-3 of the largest
    gradient entry (the truncation error is O(h^2), the rounding error ~1e-6 L / h)."""
    L = 6.0
    pos = _straddling(3, 4, L, seed=8)
    s, _ = _chain_mapping(htf, 3, 4, 2, cuda)
    u = torch.from_numpy(np.random.default_rng(2).normal(size=(6, 3)).astype(np.float32)).to(cuda)
    f = lambda p: (htf.center_of_mass(p, s, [L] * 3) * u).sum()   # noqa: E731
    x = torch.from_numpy(pos).to(cuda).requires_grad_(True)
    (g,) = torch.autograd.grad(f(x), x)
    h = 1e-2
    fd = np.zeros_like(pos)
    for a in range(pos.shape[0]):
        for c in range(3):
            xp, xm = pos.copy(), pos.copy()
            xp[a, c] += h
            xm[a, c] -= h
            fd[a, c] = (f(torch.from_numpy(xp).to(cuda)).item() - f(torch.from_numpy(xm).to(cuda)).item()) / (2 * h)
    g = g.cpu().numpy()
    assert np.abs(g - fd).max() <= 2e-3 * max(np.abs(g).max(), 1.0)


def test_nlist_backward_scatter(htf, cuda):
    """grad_pos[i] -= g_ij, grad_pos[j] += g_ij over the filled slots; nothing into the type column."""
    p, L = _cloud(300, seed=5)
    x = torch.from_numpy(p).to(cuda).requires_grad_(True)
    nl = htf.compute_nlist(x, 2.0, 32, [L] * 3, sorted=True, return_types=True)
    idx = htf.compute_nlist(x[:, :3].detach(), 2.0, 32, [L] * 3, sorted=True)[:, :, 3].long().cpu().numpy()
    u = np.random.default_rng(4).normal(size=nl.shape).astype(np.float32)
    (g,) = torch.autograd.grad((nl * torch.from_numpy(u).to(cuda)).sum(), x)
    g = g.cpu().numpy()
    ref = np.zeros((300, 4))
    filled = np.abs(nl.detach().cpu().numpy()[:, :, :3]).sum(2) > 0
    for i, s in zip(*np.nonzero(filled)):
        ref[i, :3] -= u[i, s, :3]
        ref[idx[i, s], :3] += u[i, s, :3]
    np.testing.assert_allclose(g, ref, atol=1e-5)


def test_cg_lj_forces_vs_autograd_f64(htf, cuda):
    """A CG Lennard-Jones energy on compute_nlist(center_of_mass(...)): 300 atoms -> 100 beads; compute_positions_forces
    against torch fp64 autograd of the same formula (on the same neighbor pairs), <= 2e-4 max|F|."""
    rng = np.random.default_rng(12)
    nb, L, rc, NN = 100, 5.4, 2.5, 64
    grid = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3)[:nb] * (L / 5) - L / 2
    centres = grid + rng.normal(0, 0.05, grid.shape)
    pos = (np.repeat(centres, 3, 0) + rng.normal(0, 0.15, (3 * nb, 3)))
    pos = (pos - np.round(pos / L) * L).astype(np.float32)
    s, _ = _chain_mapping(htf, nb, 3, 1, cuda)

    def energy(com_, nl):
        r2 = (nl[:, :, :3] ** 2).sum(2)
        m = r2 > 0
        rs2 = torch.where(m, r2, torch.ones_like(r2))      # (empty slots: no sqrt of zero, no gradient)
        e = torch.where(m, 4.0 * (rs2 ** -6 - rs2 ** -3), torch.zeros_like(r2))
        return e.sum() / 2

    x = torch.from_numpy(pos).to(cuda).requires_grad_(True)
    com = htf.center_of_mass(x, s, [L] * 3)
    nl = htf.compute_nlist(com, rc, NN, [L] * 3, sorted=True)
    assert (nl[:, :, 3] != 0).sum(1).max().item() < NN
    F = htf.compute_positions_forces(x, energy(com, nl))[:, :3].cpu().numpy()
    # fp64, same pairs (index column), minimum image on the fp64 centres
    x64 = torch.from_numpy(pos).double().to(cuda).requires_grad_(True)
    c64 = _torch_com(x64, s.to_dense().double(), L)
    j = nl[:, :, 3].long().detach()
    filled = (nl[:, :, :3].abs().sum(2) > 0).detach()
    d = c64[j] - c64[:, None, :]
    d = d - torch.round(d / L).detach() * L
    nl64 = d * filled[..., None]
    (g64,) = torch.autograd.grad(energy(c64, nl64), x64)
    F64 = -g64.cpu().numpy()
    assert np.abs(F - F64).max() <= 2e-4 * np.abs(F64).max()
    assert np.abs(F64).max() > 1.0


# ------------------------------------------------------------------------------------------------ 5. example 02
def _dimer_box(htf, cuda, n_side=6, a=1.6):
    """A stand-in box of six-atom molecules (two beads each), atoms on a simple-cubic lattice, bonded in runs of six."""
    from hoomd_tf_amd import standin
    g = np.stack(np.meshgrid(*[np.arange(n_side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    L = n_side * a
    pos = g * a - L / 2 + 0.25 * a
    N = pos.shape[0]
    types = (np.arange(N) % 6 == 1).astype(np.int32) * 3      # the C-C RDF of example 02 reads type 3
    system = standin.System(pos, [L] * 3, types=types, dtype=torch.float32, device=cuda)
    system.bonds = [(m * 6 + i, m * 6 + i + 1) for m in range(N // 6) for i in range(5)]
    system.vel[:, 3] = torch.from_numpy(np.tile([12.0, 1.0, 1.0, 16.0, 1.0, 1.0], N // 6).astype(np.float32)).to(cuda)
    return system, L


def test_example02_mapping_model(htf, cuda):
    import build_examples
    from hoomd_tf_amd import standin

    class MappingModel(htf.SimModel):
        def setup(self, CG_NN, cg_mapping, rcut):
            self.CG_NN, self.rcut, self.cg_mapping = CG_NN, rcut, cg_mapping
            self.avg_cg_rdf = htf.MeanTensor()
            self.avg_aa_rdf = htf.MeanTensor()

        def compute(self, nlist, positions, box):
            box_size = htf.box_size(box)
            mapped_pos = htf.center_of_mass(positions[:, :3], self.cg_mapping, box_size)
            mapped_nlist = htf.compute_nlist(mapped_pos, self.rcut, self.CG_NN, box_size, True)
            cg_rdf = htf.compute_rdf(mapped_nlist, [0.1, self.rcut])
            aa_rdf = htf.compute_rdf(nlist, [0.1, self.rcut], positions[:, 3], type_i=3, type_j=3)
            self.avg_cg_rdf.update_state(cg_rdf)
            self.avg_aa_rdf.update_state(aa_rdf)
            self.last = (positions[:, :3].detach().clone(), mapped_pos.detach().clone(), cg_rdf[0].detach().clone())
            return

    system, L = _dimer_box(htf, cuda)
    sim = standin.Simulation(system)
    index = htf.find_molecules(system)
    assert len(index) == system.N // 6
    mm = np.array([[1, 1, 1, 0, 0, 0], [0, 0, 0, 1, 1, 1]])
    cg_mapping = htf.sparse_mapping([mm for _ in index], index, system=system)
    assert tuple(cg_mapping.shape) == (2 * len(index), system.N)
    rcut = 3.0
    nlist = sim.nlist_cell()
    sim.integrate_nve(0.002).randomize_velocities(kT=0.5, seed=3)
    lj = htf.tfcompute(build_examples.LJModel(64))
    lj.attach(nlist, r_cut=2.5)
    model = MappingModel(64, CG_NN=64, cg_mapping=cg_mapping, output_forces=False, rcut=rcut, check_nlist=True)
    tfc = htf.tfcompute(model)
    tfc.attach(nlist, r_cut=rcut)
    sim.run(50)
    assert model.avg_cg_rdf.count == 50 and model.avg_aa_rdf.count == 50
    assert not tfc.graph_safe()
    pos, com, cg_rdf = (t.cpu().numpy() for t in model.last)
    # the final step's beads: the fp64 centre of mass of the positions the model saw ...
    ref_com = _com_f64(pos, cg_mapping.cpu().to_dense().double().numpy(), L)
    assert _periodic_err(com, ref_com, L).max() <= 2e-6 * L
    assert np.abs(pos - system.pos[:system.N, :3].cpu().numpy()).max() < 1.0    # (they are the step's own positions)
    # ... and the RDF over the oracle-built bead list
    ref_nl = O.compute_nlist(com, rcut, 64, [L] * 3, sorted=True)
    ref_rdf, _ = O.compute_rdf(ref_nl, [0.1, rcut])
    np.testing.assert_allclose(cg_rdf, ref_rdf, rtol=2e-5, atol=0)     # (fp32 shell volumes: numpy vs the kernel)
    same, _ = htf.compute_rdf(torch.from_numpy(ref_nl).to(cuda), [0.1, rcut])
    np.testing.assert_array_equal(cg_rdf, same.cpu().numpy())          # (the same histogram: the same bead pairs)
    assert cg_rdf.sum() > 0


def test_example02_enable_mapped_nlist(htf, cuda):
    """The same mapping through tfcompute.enable_mapped_nlist: the beads ride behind the atoms, re-mapped every step by
    htf.center_of_mass (SimModel.precompute), and the step stays eager."""
    from hoomd_tf_amd import standin

    class Beads(htf.SimModel):
        def compute(self, nlist, positions, box):
            aa, cg = self.mapped_nlist(nlist)
            return positions, cg

    system, L = _dimer_box(htf, cuda, n_side=6)
    AAN = system.N
    sim = standin.Simulation(system)
    index = htf.find_molecules(system)
    mm = np.array([[1, 1, 1, 0, 0, 0], [0, 0, 0, 1, 1, 1]])
    s = htf.sparse_mapping([mm for _ in index], index, system=system)
    B = s.shape[0]
    types = torch.zeros((B, 1), dtype=torch.float32, device=cuda)
    fn = lambda pos, Lb: torch.cat([htf.center_of_mass(pos[:, :3], s, Lb).to(pos.dtype), types.to(pos.dtype)], 1)  # noqa: E731
    tfc = htf.tfcompute(Beads(16, output_forces=False))
    aa_group, mapped_group = tfc.enable_mapped_nlist(system, fn)
    assert len(aa_group) == AAN and len(mapped_group) == B and system.N == AAN + B
    sim.integrate_nve(0.002, group=aa_group).randomize_velocities(kT=0.5, seed=1)
    tfc.attach(sim.nlist_cell(), r_cut=2.0, save_output_period=1)
    sim.run(5)
    assert not tfc.graph_safe()
    positions = tfc.outputs[0].reshape(-1, AAN + B, 4)
    dense = s.cpu().to_dense().double().numpy()
    for step in range(positions.shape[0]):
        ref = _com_f64(positions[step, :AAN, :3], dense, L)
        assert _periodic_err(positions[step, AAN:, :3], ref, L).max() <= 2e-6 * L
    assert np.abs(positions[-1, :AAN, :3] - positions[0, :AAN, :3]).max() > 1e-4
    assert tfc.outputs[1].shape[1:] == (B, 16, 4)


def test_cg_ops_keep_force_model_eager(htf, cuda):
    """A force model that also observes its beads (center_of_mass -> compute_nlist -> compute_rdf -> MeanTensor) must not be
    replaced by the one-kernel plan: the CG observable is updated at every step and the step is never graph-replayed."""
    from hoomd_tf_amd import standin

    class LJWithBeads(htf.SimModel):
        def setup(self, mapping):
            self.mapping = mapping
            self.avg = htf.MeanTensor()

        def compute(self, nlist, positions, box):
            bs = htf.box_size(box)
            beads = htf.compute_nlist(htf.center_of_mass(positions[:, :3], self.mapping, bs), 3.0, 32, bs, True)
            self.avg.update_state(htf.compute_rdf(beads, [0.1, 3.0]))
            rinv = htf.nlist_rinv(nlist)
            inv_r6 = rinv ** 6
            return htf.compute_nlist_forces(nlist, htf.reduce_sum(2.0 * (inv_r6 * inv_r6 - inv_r6), axis=1))

    system, L = _dimer_box(htf, cuda, n_side=6)
    sim = standin.Simulation(system)
    index = htf.find_molecules(system)
    s = htf.sparse_mapping([np.array([[1, 1, 1, 0, 0, 0], [0, 0, 0, 1, 1, 1]]) for _ in index], index, system=system)
    sim.integrate_nve(0.002).randomize_velocities(kT=0.5, seed=2)
    model = LJWithBeads(64, mapping=s)
    tfc = htf.tfcompute(model)
    tfc.attach(sim.nlist_cell(), r_cut=2.5)
    sim.run(12)
    assert model.avg.count == 12
    assert not tfc.graph_safe() and sim._graph_cycle() == 0
