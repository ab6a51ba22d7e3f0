"""The cell-binned route of ``compute_nlist`` (csrc/nlist_cells.hip) against the all-pairs route and the numpy oracle, bit for
bit: every geometry that stresses the binning (exactly 3 cells, many cells, anisotropic boxes, points on cell faces and
exactly r_cut apart, positions shifted by whole boxes or far outside them, empty and crowded cells), exclusions, large M,
determinism, gradients and the route rule of ``cgmap._nlist_route``."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import htf_oracle as O
from test_gpu_cg import _bits, _cloud, _nlist_ref

pytestmark = pytest.mark.gpu

NNS = (1, 16, 64, 256)


@contextlib.contextmanager
def _route(min_m):
    from hoomd_tf_amd import cgmap
    old = cgmap.NLIST_CELLS_MIN_M
    cgmap.NLIST_CELLS_MIN_M = min_m
    try:
        yield cgmap
    finally:
        cgmap.NLIST_CELLS_MIN_M = old


def _both(htf, x, r_cut, NN, L, **kw):
    """(cell route, all-pairs route) of the same call, as numpy."""
    with _route(0) as cgmap:
        assert cgmap._nlist_route(x.shape[0], L, r_cut) == "cells"
        cells = htf.compute_nlist(x, r_cut, NN, L, **kw).cpu().numpy()
    with _route(1 << 62) as cgmap:
        assert cgmap._nlist_route(x.shape[0], L, r_cut) == "all-pairs"
        pairs = htf.compute_nlist(x, r_cut, NN, L, **kw).cpu().numpy()
    return cells, pairs


def _same(a, b):
    assert a.shape == b.shape
    np.testing.assert_array_equal(a[..., 3], b[..., 3])
    np.testing.assert_array_equal(_bits(a[..., :3]), _bits(b[..., :3]))


def _check(htf, cuda, p, L, r_cut, NN, sorted_, types, oracle_rows=None, excl=None):
    """cells == all pairs on every row, and == the restatement of the oracle on ``oracle_rows`` (all rows if None)."""
    x = torch.from_numpy(p if types else np.ascontiguousarray(p[:, :3])).to(cuda)
    kw = dict(sorted=sorted_, return_types=types)
    if excl is not None:
        kw["exclusion_matrix"] = torch.from_numpy(excl).to(cuda)
    cells, pairs = _both(htf, x, r_cut, NN, L, **kw)
    _same(cells, pairs)
    rows = np.arange(p.shape[0]) if oracle_rows is None else oracle_rows
    ref = _nlist_ref(p, r_cut, NN, L, sorted_, types, excl=excl, rows=rows)
    _same(cells[rows], ref)
    return cells


def _uniform(M, L, seed, types=4):
    rng = np.random.default_rng(seed)
    L = np.asarray(L, np.float32)
    p = (rng.random((M, 3)) * L).astype(np.float32)
    t = rng.integers(0, types, M).astype(np.float32)
    return np.concatenate([p, t[:, None]], 1).astype(np.float32)


@pytest.mark.parametrize("NN", NNS)
@pytest.mark.parametrize("sorted_", [True, False])
def test_three_cells_per_dimension(htf, cuda, NN, sorted_):
    from hoomd_tf_amd import cgmap
    p, L = _cloud(700, seed=NN + 3 * sorted_, L=7.0)
    assert cgmap._cell_grid(700, [7.0] * 3, np.float32(2.0)) == (3, 3, 3)
    _check(htf, cuda, p, [L] * 3, 2.0, NN, sorted_, types=NN % 2 == 0)


@pytest.mark.parametrize("NN", NNS)
@pytest.mark.parametrize("sorted_", [True, False])
def test_many_cells(htf, cuda, NN, sorted_):
    from hoomd_tf_amd import cgmap
    M, L = 20000, 30.0
    p = _uniform(M, [L] * 3, seed=NN)
    grid = cgmap._cell_grid(M, [L] * 3, np.float32(1.6))
    assert min(grid) >= 15
    rows = np.concatenate([np.arange(0, M, 211), [M - 1]])
    _check(htf, cuda, p, [L] * 3, 1.6, NN, sorted_, types=not sorted_, oracle_rows=rows)


@pytest.mark.parametrize("NN", NNS)
def test_anisotropic_box(htf, cuda, NN):
    from hoomd_tf_amd import cgmap
    L = [31.0, 9.5, 14.25]
    p = _uniform(5000, L, seed=7)
    p[:, :3] -= np.float32(7.0)                     # partly outside [0, L)
    grid = cgmap._cell_grid(5000, L, np.float32(2.5))
    assert grid[0] > grid[2] > grid[1] == 3
    _check(htf, cuda, p, L, 2.5, NN, True, types=True, oracle_rows=np.arange(0, 5000, 7))
    _check(htf, cuda, p, L, 2.5, NN, False, types=False, oracle_rows=np.arange(3, 5000, 7))


@pytest.mark.parametrize("NN", NNS)
def test_lattice_exactly_r_cut_apart_and_cell_faces(htf, cuda, NN):
    """A simple-cubic lattice of spacing r_cut (exact in fp32, as every difference): six neighbors of every lattice point
    are exactly at d = r_cut, all of them tied.  Plus points on the cell faces k L / n (and one ulp either side)."""
    from hoomd_tf_amd import cgmap
    L, r = 16.0, 1.0
    g = np.arange(0, 16, 1.0, dtype=np.float32)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    n = cgmap._cell_grid(lat.shape[0] + 300, [L] * 3, np.float32(r))[0]
    faces = np.float32(L) / np.float32(n) * np.arange(n, dtype=np.float32)
    rng = np.random.default_rng(1)
    extra = rng.random((300, 3)).astype(np.float32) * np.float32(L)
    pick = rng.integers(0, n, (300, 2))
    extra[:, 0] = faces[pick[:, 0]]
    extra[:100, 1] = np.nextafter(faces[pick[:100, 1]], np.float32(-1))
    extra[100:200, 1] = np.nextafter(faces[pick[100:200, 1]], np.float32(100))
    extra[200:, 2] = faces[pick[200:, 1]]
    p = np.concatenate([lat, extra]).astype(np.float32)
    p = np.concatenate([p, (np.arange(p.shape[0]) % 3).astype(np.float32)[:, None]], 1)
    rows = np.concatenate([np.arange(0, lat.shape[0], 37), np.arange(lat.shape[0], p.shape[0])])
    cells = _check(htf, cuda, p, [L] * 3, r, NN, True, types=True, oracle_rows=rows)
    if NN >= 16:
        d = np.sqrt((cells[:lat.shape[0], :, :3].astype(np.float64) ** 2).sum(2))
        assert ((d == r).sum(1) >= 6).all()                                           # six neighbors at exactly r_cut


@pytest.mark.parametrize("shift", [0, 1, -1, 2, -2])
@pytest.mark.parametrize("NN", [16, 256])
def test_shifted_by_whole_boxes(htf, cuda, shift, NN):
    L = [12.0, 12.0, 15.0]
    p = _uniform(3000, L, seed=5)
    p[: 50, :3] = 0.0                               # (exact distance ties across the boundary)
    p[: 50, 0] = np.arange(50, dtype=np.float32) * np.float32(0.25)
    p[:, :3] += np.float32(shift) * np.asarray(L, np.float32)
    rows = np.arange(0, 3000, 5)
    _check(htf, cuda, p, L, 2.0, NN, True, types=False, oracle_rows=rows)
    _check(htf, cuda, p, L, 2.0, NN, False, types=True, oracle_rows=rows)


@pytest.mark.parametrize("NN", [16, 64])
def test_far_and_non_finite_positions(htf, cuda, NN):
    """Rows beyond 64 box lengths, and not finite ones, fall into the extra cell: still the all-pairs list."""
    L = [10.0] * 3
    p = _uniform(2000, L, seed=9)
    p[:20, :3] += np.float32(1000.0)                # 100 L away: the extra cell
    p[20:40, 0] = p[:20, 0] + np.float32(0.5)       # ... with neighbors of their own there
    p[20:40, 1:3] = p[:20, 1:3]
    p[40:45, :3] -= np.float32(640.0)               # exactly 64 L: still binned
    p[45, 0] = np.nan
    p[46, 1] = np.inf
    x = torch.from_numpy(p).to(cuda)
    for sorted_ in (True, False):
        cells, pairs = _both(htf, x, 2.0, NN, L, sorted=sorted_, return_types=True)
        _same(cells, pairs)
        assert np.all(cells[45:47] == 0) and np.any(cells[:20, :, :3] != 0)


@pytest.mark.parametrize("NN", NNS)
def test_empty_cells_and_one_crowded_cell(htf, cuda, NN):
    """Half the points inside one cell, the rest sparse over a box of mostly empty cells (more cells than points: the
    grid is capped)."""
    from hoomd_tf_amd import cgmap
    M, L, r = 4000, 60.0, 2.0
    rng = np.random.default_rng(NN)
    p = _uniform(M, [L] * 3, seed=NN + 1)
    p[: M // 2, :3] = (np.float32(31.0) + rng.random((M // 2, 3)) * np.float32(0.9)).astype(np.float32)
    grid = cgmap._cell_grid(M, [L] * 3, np.float32(r))
    assert np.prod(grid) <= M
    rows = np.concatenate([np.arange(0, M // 2, 50), np.arange(M // 2, M, 3)])
    _check(htf, cuda, p, [L] * 3, r, NN, True, types=False, oracle_rows=rows)
    _check(htf, cuda, p, [L] * 3, r, NN, False, types=True, oracle_rows=rows[::3])


@pytest.mark.parametrize("sorted_,types", [(True, False), (False, True)])
def test_exclusions(htf, cuda, sorted_, types):
    M = 1000
    p, L = _cloud(M, seed=11)
    em = np.random.default_rng(3).random((M, M)) < 0.2          # not symmetric: applied both ways
    for NN in NNS:
        _check(htf, cuda, p, [L] * 3, 2.0, NN, sorted_, types, excl=em)


@pytest.mark.parametrize("NN,sorted_", [(64, True), (256, False)])
def test_131072_sampled_rows(htf, cuda, NN, sorted_):
    M = 131072
    L = float(np.float32(M ** (1 / 3)))
    p = _uniform(M, [L] * 3, seed=NN)
    rows = np.concatenate([np.arange(0, M, 1031), [M - 1]])
    _check(htf, cuda, p, [L] * 3, 2.5, NN, sorted_, types=sorted_, oracle_rows=rows)


def test_vs_oracle_small(htf, cuda):
    """The oracle itself (not the restatement) on the cell route."""
    p, L = _cloud(1000, seed=4)
    x = torch.from_numpy(p).to(cuda)
    with _route(0):
        got = htf.compute_nlist(x, 2.0, 64, [L] * 3, sorted=True, return_types=True).cpu().numpy()
    ref = O.compute_nlist(p, 2.0, 64, [L] * 3, sorted=True, return_types=True)
    _same(got[:, :ref.shape[1]], ref)


def test_two_calls_same_bits(htf, cuda):
    p = _uniform(50000, [37.0] * 3, seed=2)
    p[:20000, :3] = np.float32(3.0) + np.random.default_rng(0).random((20000, 3)).astype(np.float32)
    x = torch.from_numpy(p).to(cuda)
    with _route(0):
        a = htf.compute_nlist(x, 2.0, 64, [37.0] * 3, sorted=True).cpu().numpy()
        b = htf.compute_nlist(x, 2.0, 64, [37.0] * 3, sorted=True).cpu().numpy()
    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))


def test_gradients_equal_all_pairs(htf, cuda):
    p = _uniform(3000, [14.0] * 3, seed=8)
    w = torch.from_numpy(np.random.default_rng(1).standard_normal((3000, 32, 4)).astype(np.float32)).to(cuda)
    grads = []
    for min_m in (0, 1 << 62):
        x = torch.from_numpy(p).to(cuda).requires_grad_(True)
        with _route(min_m):
            nl = htf.compute_nlist(x, 2.2, 32, [14.0] * 3, sorted=True, return_types=True)
        (nl * w).sum().backward()
        grads.append(x.grad.cpu().numpy())
    assert np.any(grads[0][:, :3] != 0)
    np.testing.assert_allclose(grads[0], grads[1], rtol=1e-5, atol=1e-5)


def test_route_rule(htf, cuda):
    """The rule with the measured threshold: cells from NLIST_CELLS_MIN_M on when every dimension fits 3 cells."""
    from hoomd_tf_amd import cgmap
    m0 = cgmap.NLIST_CELLS_MIN_M
    big = max(m0, 131072)
    assert cgmap._nlist_route(big, [40.0] * 3, 3.0) == "cells"
    assert cgmap._nlist_route(big, [7.0, 7.0, 7.0], 2.0) == "cells"
    assert cgmap._nlist_route(big, [40.0, 40.0, 5.9], 2.0) == "all-pairs"     # 2 cells along z
    assert cgmap._nlist_route(big, [40.0] * 3, 14.0) == "all-pairs"
    assert cgmap._nlist_route(big, [6.0] * 3, 2.0) == "all-pairs"              # 6 / (2 + margin) < 3
    assert cgmap._nlist_route(big, [40.0] * 3, float("nan")) == "all-pairs"
    if m0 > 1:
        assert cgmap._nlist_route(m0 - 1, [40.0] * 3, 3.0) == "all-pairs"
    # the cases of test_gpu_cg.py at their sizes
    for M, L, r in ((1000, 12.0, 2.0), (20000, 40.0, 3.0)):
        assert cgmap._nlist_route(M, [L] * 3, r) == ("cells" if M >= m0 else "all-pairs")
    # a device box takes the same route (read back once)
    x = torch.from_numpy(_uniform(2000, [20.0] * 3, seed=1)).to(cuda)
    Ld = torch.tensor([20.0] * 3, device=cuda)
    with _route(0):
        a = htf.compute_nlist(x, 2.0, 16, Ld, sorted=True).cpu().numpy()
    with _route(1 << 62):
        b = htf.compute_nlist(x, 2.0, 16, [20.0] * 3, sorted=True).cpu().numpy()
    _same(a, b)
