"""The per-cell neighbor search (``build_nlist_cells_kernel``, grids of >= 1 024 cells) at the shapes where its bookkeeping can go
wrong: batches of eight particles per cell and wave, walks whose length sits at a trip (64 candidates), a bitmap word or the
bitmap's capacity (2 048 candidates: beyond it the run of a candidate is searched for, below it read from the bitmap), runs that
are empty in the middle and at the end of the table, a particle that is the first or the last candidate of a trip, a home run that
wraps around the box, rows longer than the pitch, grids without the image shift, a non-periodic axis, the type split, ghosts.

Every system is a few thousand particles on a grid of cells 0.5 wide, r_list = 1, rebuilt by ``htfs_rebuild_nlist`` into
sentinel-filled arrays and compared with the fp64 brute-force list of ``helpers.brute_nlist`` on the positions as stored.
fp64: the sets are equal.  fp32: pairs whose fp64 distance lies within 1e-5 of r_list are left out of the comparison, at most
six per system (asserted on the oracle alone first; ``test_cell_nlist_random_boxes_match_brute_force`` has the same cap).
The order inside a row: a child process per search kernel on the variants build, rows equal entry for entry.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import brute_nlist, min_image_np, variants_env

R_LIST, W, SW = 1.0, 0.5, 2     # list radius, cell width, stencil half-width
NEAR, NEAR_MAX = 1e-5, 6
SENTINEL = -7


# ------------------------------------------------------------------------------------------------ systems (CPU, seeded)
def _in_cell(rng, grid, cell, k, tight=False):
    """k positions inside cell (cx, cy, cz) of the grid (taken modulo the grid), away from its faces.  ``tight``: all within 0.005
    of one point of the cell -- thousands of candidates in one walk, and still only a few pairs of the system near r_list."""
    g = np.asarray(grid)
    c = np.mod(np.asarray(cell), g)
    u = rng.uniform(0.25, 0.75, 3) + rng.uniform(-0.01, 0.01, (k, 3)) if tight else rng.uniform(0.1, 0.9, (k, 3))
    return (c + u) * W - 0.5 * g * W


def _background(rng, grid, k, keep_out=()):
    """k uniformly placed positions in none of the cells ``keep_out``."""
    g = np.asarray(grid)
    out = np.zeros((0, 3))
    ban = {tuple(np.mod(c, g)) for c in keep_out}
    while len(out) < k:
        x = rng.uniform(-0.5, 0.5, (k, 3)) * g * W
        c = np.floor(x / W + 0.5 * g).astype(int)
        ok = np.array([tuple(ci) not in ban for ci in c])
        out = np.concatenate([out, x[ok]])
    return out[:k]


def _cluster(rng, grid, home, T, B, m=2, left=0, tight=False):
    """A walk of exactly T candidates for cell ``home`` (nothing else within its stencil): B in the stencil row (dy, dz) =
    (-2, 0), which the walk visits before the home row; ``left`` in the home row's cell at x - 1; m in the cell itself -- they are
    candidates B + left .. B + left + m - 1 of the walk; the rest behind them, in the home row at x + 1 and in rows (1, 0), (0, 1)
    and (-2, 2).  Rows (-1, 0) and (2, 2) -- the middle and the end of the table -- stay empty."""
    h = np.asarray(home)
    parts = [_in_cell(rng, grid, h, m, tight), _in_cell(rng, grid, h + [-1, 0, 0], left, tight)]
    for k, dx in zip(np.bincount(rng.integers(0, 5, B), minlength=5), range(-2, 3)):
        parts.append(_in_cell(rng, grid, h + [dx, -2, 0], k, tight))
    after = [(1, 0, 0), (-2, 1, 0), (2, 1, 0), (0, 0, 1), (-1, -2, 2)]
    A = T - B - m - left
    assert A >= 0
    for k, off in zip(np.bincount(rng.integers(0, len(after), A), minlength=len(after)), after):
        parts.append(_in_cell(rng, grid, h + list(off), k, tight))
    return np.concatenate(parts)


def _case(pos, grid, tdt, N=None, periodic=(1, 1, 1), types=None, type_split=-1, pitch=None, inert=()):
    return dict(pos=np.asarray(pos, dtype=np.float64), grid=tuple(grid), tdt=tdt, N=len(pos) if N is None else N,
                periodic=tuple(periodic), types=types, type_split=type_split, pitch=pitch, inert=tuple(inert))


def _make(name):
    f32, f64 = torch.float32, torch.float64
    kind, _, prec = name.rpartition("-")
    tdt = f64 if prec == "f64" else f32
    rng = np.random.default_rng(sum(map(ord, kind)))
    if kind in ("batches2", "batches1"):
        # cells of 1, 8, 9, 16, 17 and 25 particles: one batch, a full one, a second, two full ones, a third (with two waves per
        # cell -- 16^3 = 4 096 cells -- the one that returns to wave 0), a fourth; 24^3 = 13 824 cells: one wave per cell.
        # One dense cell sits at the last x, its home run wrapping around the box.
        n = 16 if kind == "batches2" else 24
        grid = (n, n, n)
        cells = [(2, 2, 2), (7, 2, 2), (n - 1, 2, 2), (2, 8, 8), (7, 8, 8), (12, 8, 8)]
        parts = [_in_cell(rng, grid, c, k) for c, k in zip(cells, (1, 8, 9, 16, 17, 25))]
        parts.append(_background(rng, grid, 1500 if n == 16 else 2200, keep_out=cells))
        return _case(np.concatenate(parts), grid, tdt)
    if kind == "walks":
        grid = (16, 16, 16)
        return _case(np.concatenate([_cluster(rng, grid, h, *s) for h, s in zip(WALK_HOMES, WALK_SPECS)]), grid, tdt)
    if kind.startswith("long"):
        # a walk at the bitmap's capacity and one past it, beside a short one
        grid = (16, 16, 16)
        rng = np.random.default_rng(LONG_SEED)
        pos = np.concatenate([_cluster(rng, grid, LONG_HOME, int(kind[4:]), int(kind[4:]) // 2, 4, 9, tight=True), _cluster(rng, grid, (12, 2, 2), 70, 10)])
        return _case(pos, grid, tdt, pitch=1536)
    if kind in ("noshift", "open_z"):
        # 6 cells along a periodic axis: no image shift, rint() per pair; a non-periodic axis: the stencil ends at the wall
        grid, per = ((6, 14, 14), (1, 1, 1)) if kind == "noshift" else ((14, 14, 6), (1, 1, 0))
        return _case(_background(rng, grid, 2400), grid, tdt, periodic=per)
    if kind == "types":
        grid = (16, 16, 16)
        pos = np.concatenate([_background(rng, grid, 2000), _in_cell(rng, grid, (3, 3, 3), 21)])
        return _case(pos, grid, tdt, types=(rng.random(len(pos)) < 0.4).astype(np.int32), type_split=1)
    if kind == "ghosts":
        # 1 800 rows + 700 ghosts behind them: 400 in cells no row sits in (x cells 12..15), 300 among the rows -- and a cell of
        # 12 whose second batch mixes both; a few inert rows (x = NaN), which are in no cell
        grid = (16, 16, 16)
        loc = _background(rng, grid, 1800)
        loc[:, 0] = (loc[:, 0] + 4.0) * 0.75 - 4.0            # x cells 0..11
        far = _background(rng, grid, 400)
        far[:, 0] = (far[:, 0] + 4.0) * 0.25 + 2.0            # x cells 12..15
        mix = _background(rng, grid, 294)
        mix[:, 0] = (mix[:, 0] + 4.0) * 0.75 - 4.0
        loc[:6] = _in_cell(rng, grid, (4, 4, 4), 6)
        pos = np.concatenate([loc, far, mix, _in_cell(rng, grid, (4, 4, 4), 6)])
        return _case(pos, grid, tdt, N=1800, inert=(17, 500, 1799))
    raise KeyError(name)


# (T, B, m, left): a walk's length and where the cell's own m particles sit in it (_cluster): fewer than a trip of 64, exactly one
# and two trips, 64 k + 1; the cell's own as the first candidates of the walk, as the last of a trip and the first of the next
WALK_SPECS = [(1, 0, 1, 0), (2, 0, 2, 0), (63, 30, 2, 1), (64, 0, 2, 0), (65, 20, 2, 2), (127, 50, 2, 0), (128, 126, 2, 0),
              (129, 64, 2, 0), (130, 60, 2, 3), (192, 100, 2, 5), (193, 191, 2, 0), (257, 120, 3, 7)]
# clusters out of one another's stencils; x = 0: the home run wraps around the box
WALK_HOMES = [(x, y, z) for z in (2, 8, 13) for y in (2, 8, 13) for x in (0, 5, 10)]
LONG_HOME, LONG_SEED = (5, 8, 8), 2   # (the seed: chosen on the CPU for at most six borderline pairs)
KINDS = ["batches2", "batches1", "walks", "long2048", "long2049", "noshift", "open_z", "types", "ghosts"]
NAMES = [k + "-" + p for k in KINDS for p in ("f32", "f64")]


# ------------------------------------------------------------------------------------------------ the rebuild
class _Built:
    """One ``htfs_rebuild_nlist`` of a case into sentinel-filled arrays."""

    def __init__(self, htf, dev, case, pitch, rebuilds=1):
        from hoomd_tf_amd import ops
        g, tdt, N = case["grid"], case["tdt"], case["N"]
        Ntot = len(case["pos"])
        ncell = int(np.prod(g))
        types = np.zeros(Ntot, np.int32) if case["types"] is None else case["types"]
        self.pos = ops.stuff_types(torch.from_numpy(case["pos"]).to(dev), torch.from_numpy(types).to(dev), tdt)
        for i in case["inert"]:
            self.pos[i, 0] = float("nan")
        self.N, self.Ntot, self.pitch, self.dev = N, Ntot, pitch, dev
        self.code = htf._lib.HTF_F32 if tdt == torch.float32 else htf._lib.HTF_F64
        i32 = dict(dtype=torch.int32, device=dev)
        self.bufs = dict(cell_of=torch.empty(Ntot, **i32), scratch=torch.zeros(2 * ncell + 2 + Ntot, **i32),
                         cell_start=torch.empty(ncell + 1, **i32), order=torch.empty(Ntot, **i32),
                         pos_sorted=torch.zeros((Ntot, 4), dtype=tdt, device=dev), ranges=torch.zeros(4 * ncell * (2 * SW + 1) ** 2, **i32),
                         n_neigh=torch.full((N,), SENTINEL, **i32), head_list=torch.full((N,), SENTINEL, **i32),
                         nlist=torch.full((N * pitch,), SENTINEL, **i32), ref=torch.zeros((N, 4), dtype=tdt, device=dev))
        self.stat = torch.zeros(2, **i32)   # [largest row, rebuilds]
        self.disp = torch.zeros(1, dtype=torch.float32, device=dev)
        d = self.desc = htf._lib.Nlist()
        half = 0.5 * W * np.asarray(g, dtype=np.float64)
        d.box = htf._lib.make_box(np.array([-half, half, [0.0] * 3]), case["periodic"])
        d.r_list, d.pitch, d.type_split = R_LIST, pitch, case["type_split"]
        d.ncell3[:] = list(g)
        d.stencil3[:] = [SW] * 3
        d.image_L[:] = [0.0] * 3
        for k, v in self.bufs.items():
            setattr(d, k, v.data_ptr())
        d.max_neigh, d.counter = self.stat.data_ptr(), self.stat.data_ptr() + 4
        self.htf = htf
        for _ in range(rebuilds):
            self.rebuild()

    def _stream(self):
        from hoomd_tf_amd.ops import raw_stream
        return C.c_void_p(raw_stream(self.dev.index))

    def rebuild(self):
        lib = self.htf._lib
        lib.check(lib.lib.htfs_rebuild_nlist(C.byref(self.desc), self.pos.data_ptr(), self.code, self.N, self.Ntot, 0, self._stream()))
        torch.cuda.synchronize()

    def check_rebuild(self, thr2):
        lib = self.htf._lib
        lib.check(lib.lib.htfs_check_rebuild_nlist(C.byref(self.desc), self.pos.data_ptr(), self.code, self.N, self.Ntot, 0,
                                                   self.disp.data_ptr(), float(thr2), self.stat.data_ptr(), None, self._stream()))
        torch.cuda.synchronize()

    def arrays(self):
        return (self.bufs["n_neigh"].cpu().numpy().copy(), self.bufs["head_list"].cpu().numpy().copy(),
                self.bufs["nlist"].cpu().numpy().reshape(self.N, self.pitch).copy())


# ------------------------------------------------------------------------------------------------ the oracle
_ORACLE = {}


def _oracle(name, stored):
    """(rows, near): the fp64 brute-force rows (index-sorted) of the case on the positions as stored, types applied, and the set
    of pairs (i, j) whose distance lies within NEAR of r_list -- computed once per case."""
    if name in _ORACLE:
        return _ORACLE[name]
    case = _make(name)
    N = case["N"]
    p = stored.astype(np.float64)
    live = ~np.isnan(p[:, 0])
    q = np.where(live[:, None], p, 0.0)
    L = np.where(case["periodic"], W * np.asarray(case["grid"]), 1e9)         # a non-periodic axis: no image ever nearer
    bn, bh, bl = brute_nlist(q, L, R_LIST, n_local=N)
    rows = [np.sort(bl[int(bh[i]): int(bh[i]) + int(bn[i])]).astype(np.int64) for i in range(N)]
    rows = [r[live[r]] for r in rows]   # an inert row is nobody's neighbor
    if case["types"] is not None:
        side = case["types"] >= case["type_split"]
        rows = [r[side[r] == side[i]] for i, r in enumerate(rows)]
    near = set()
    for i0 in range(0, N, 512):
        d = min_image_np(q[None, :, :] - q[i0: i0 + 512, None, :], L)
        r = np.sqrt(np.sum(d * d, axis=2))
        for a, b in zip(*np.nonzero(np.abs(r - R_LIST) < NEAR)):
            if live[a + i0] and live[b]:
                near.add((int(a) + i0, int(b)))
    _ORACLE[name] = (rows, near)
    return rows, near


def _pitch_for(case):
    return case["pitch"] or 704


def _compare(name, case, stored, nn, rows_got):
    """rows_got[i]: the first nn[i] entries of row i.  -> the oracle's rows."""
    rows, near = _oracle(name, stored)
    f32 = case["tdt"] == torch.float32
    if f32:   # (on the oracle alone, before anything of the kernel's is looked at)
        assert len({tuple(sorted(pr)) for pr in near}) <= NEAR_MAX, "the seeded system has too many borderline pairs: %r" % (sorted(near),)
    for i, (g, r) in enumerate(zip(rows_got, rows)):
        if i in case["inert"]:
            continue
        assert len(set(g.tolist())) == len(g) and i not in set(g.tolist()), "row %d holds a duplicate or the particle itself" % i
        gs, rs = set(g.tolist()), set(r.tolist())
        if f32:
            skip = {j for (a, j) in near if a == i}
            gs, rs = gs - skip, rs - skip
        assert gs == rs, "%s row %d: %d extra, %d missing" % (name, i, len(gs - rs), len(rs - gs))
    return rows


# ------------------------------------------------------------------------------------------------ tests
def _walk(case, home):
    """(walk length of cell ``home``, walk numbers of its own particles, population of each stencil row in table order), from the
    cell populations: rows (dz, dy) in table order, in a row the main x-run (the cells inside the box) before the wrapped one."""
    g = np.asarray(case["grid"])
    cell = np.floor(case["pos"] / W + 0.5 * g).astype(int)
    pop = np.zeros(case["grid"], dtype=int)
    np.add.at(pop, tuple(cell.T), 1)
    hx, hy, hz = home
    rows, before = [], None
    for dz in range(-SW, SW + 1):
        for dy in range(-SW, SW + 1):
            xs = [x for x in range(hx - SW, hx + SW + 1) if 0 <= x < g[0]] + [x % g[0] for x in range(hx - SW, hx + SW + 1) if not 0 <= x < g[0]]
            if dz == 0 and dy == 0:
                before = sum(rows) + sum(pop[x, hy, hz] for x in xs[: xs.index(hx)])
            rows.append(sum(pop[x, (hy + dy) % g[1], (hz + dz) % g[2]] for x in xs))
    return sum(rows), [before + k for k in range(pop[hx, hy, hz])], rows


def test_the_seeded_walks_are_the_shapes_they_stand_for():
    """(No GPU: the inputs alone.)  Walk lengths as listed, empty runs in the middle and at the end of the table, the cell's own
    particles as the first and the last candidate of a trip, a home run that wraps; the long walks at 2 048 and 2 049."""
    case = _make("walks-f32")
    lanes = set()
    for home, (T, B, m, left) in zip(WALK_HOMES, WALK_SPECS):
        total, own, rows = _walk(case, home)
        assert total == T and len(own) == m, (home, total, own)
        lanes |= {q % 64 for q in own}
        assert rows[10] == B and rows[11] == 0 and rows[24] == 0 and sum(rows[12:]) == T - B and sum(rows[:10]) == 0
        if T - B - m - left > 30:
            assert rows[13] > 0 and rows[17] > 0 and rows[20] > 0
    assert {0, 63} <= lanes
    assert any(h[0] == 0 and s[0] > 60 for h, s in zip(WALK_HOMES, WALK_SPECS))
    for T in (2048, 2049):
        assert _walk(_make("long%d-f32" % T), LONG_HOME)[0] == T
    for kind, n in (("batches2", 16), ("batches1", 24)):
        case = _make(kind + "-f32")
        assert [len(_walk(case, c)[1]) for c in [(2, 2, 2), (7, 2, 2), (n - 1, 2, 2), (2, 8, 8), (7, 8, 8), (12, 8, 8)]] == [1, 8, 9, 16, 17, 25]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_rows_match_brute_force(htf, cuda, name):
    case = _make(name)
    assert int(np.prod(case["grid"])) >= 1024
    b = _Built(htf, cuda, case, _pitch_for(case))
    nn, head, nl = b.arrays()
    stored = b.pos[:, :3].cpu().numpy()
    rows = _compare(name, case, stored, nn, [nl[i, : max(nn[i], 0)] for i in range(b.N)])
    keep = np.array([i not in case["inert"] for i in range(b.N)])
    assert np.array_equal(head[keep], (np.arange(b.N) * b.pitch)[keep])
    assert int(nn[keep].max()) <= b.pitch and int(b.stat[0]) == int(nn[keep].max()) and int(b.stat[1]) == 1
    # nothing behind a row's entries, nothing for an inert row
    assert all(np.all(nl[i, max(nn[i], 0):] == SENTINEL) for i in range(b.N))
    assert max(len(r) for r in rows) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_rows_longer_than_the_pitch_are_cut_not_spilled(htf, cuda, prec):
    """The walks system holds rows from empty to a few hundred entries.  At a pitch far below them, at the median row, one below
    the longest row, at it and one above: n_neigh is clamped to the pitch, the status word reports the true count, the entries
    below the pitch are the first entries of the full row, and nothing is written past them."""
    case = _make("walks-" + prec)
    full = _Built(htf, cuda, case, 704)
    fn, _, fl = full.arrays()
    longest = int(fn.max())
    assert fn.min() == 0 and 8 < int(np.median(fn)) < longest - 1 and longest < 704   # (five different pitches)
    for pitch in (8, int(np.median(fn)), longest - 1, longest, longest + 1):
        b = _Built(htf, cuda, case, pitch)
        nn, head, nl = b.arrays()
        assert np.array_equal(nn, np.minimum(fn, pitch)) and np.array_equal(head, np.arange(b.N) * pitch)
        assert int(b.stat[0]) == longest
        for i in range(b.N):
            assert np.array_equal(nl[i, : nn[i]], fl[i, : nn[i]]) and np.all(nl[i, nn[i]:] == SENTINEL), (pitch, i)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["batches2-f32", "ghosts-f64"])
def test_a_second_rebuild_gives_the_same_bits_and_a_closed_gate_nothing(htf, cuda, name):
    case = _make(name)
    once, twice = _Built(htf, cuda, case, 96), _Built(htf, cuda, case, 96, rebuilds=2)
    for a, b in zip(once.arrays(), twice.arrays()):
        assert np.array_equal(a, b)
    assert int(twice.stat[1]) == 2 and int(twice.stat[0]) == int(once.stat[0])
    # behind a closed gate (no row has moved from the reference positions the rebuild committed): everything stays as it is
    for k in ("n_neigh", "head_list", "nlist"):
        twice.bufs[k].fill_(SENTINEL)
    twice.stat[0] = 12345
    twice.check_rebuild(1e-3)
    assert all(bool((twice.bufs[k] == SENTINEL).all()) for k in ("n_neigh", "head_list", "nlist"))
    assert twice.stat.tolist() == [12345, 2]
    # ... and an open one rebuilds
    twice.check_rebuild(-1.0)
    for a, b in zip(once.arrays(), twice.arrays()):
        assert np.array_equal(a, b)
    assert twice.stat.tolist() == [int(once.stat[0]), 3]


def _dump(path):
    """Child process: every case through whichever search kernel the environment forces -> n_neigh, rows and stored positions."""
    import hoomd_tf_amd as htf
    dev = torch.device("cuda:0")
    out = {}
    for name in NAMES:
        case = _make(name)
        b = _Built(htf, dev, case, _pitch_for(case))
        nn, _, nl = b.arrays()
        out[name + "/nn"], out[name + "/nl"], out[name + "/pos"] = nn, nl, b.pos[:, :3].cpu().numpy()
    np.savez(path, **out)


@pytest.mark.gpu
def test_rows_come_out_in_the_order_of_the_walk_per_particle(cuda, tmp_path):
    """Both search kernels, each forced in a child process on the variants build (the switches exist there only), on every
    system above: the rows agree entry for entry.  A row that holds a borderline pair (fp32) may differ in that pair -- the image
    shift is applied to the candidate by one kernel and to the particle by the other -- and is compared as a set."""
    got = {}
    for kernel in ("HTFS_NLIST_PER_CELL", "HTFS_NLIST_PER_PARTICLE"):
        path = str(tmp_path / (kernel + ".npz"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=variants_env(**{kernel: "1"}), capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        got[kernel] = np.load(path)
    a, b = got["HTFS_NLIST_PER_CELL"], got["HTFS_NLIST_PER_PARTICLE"]
    for name in NAMES:
        case = _make(name)
        assert np.array_equal(a[name + "/pos"], b[name + "/pos"], equal_nan=True)
        _, near = _oracle(name, a[name + "/pos"])
        loose = {i for (i, _) in near} if case["tdt"] == torch.float32 else set()
        na, nb, la, lb = a[name + "/nn"], b[name + "/nn"], a[name + "/nl"], b[name + "/nl"]
        for i in range(case["N"]):
            if i in case["inert"]:
                continue
            if i in loose:
                skip = {j for (x, j) in near if x == i}
                assert set(la[i, : na[i]].tolist()) - skip == set(lb[i, : nb[i]].tolist()) - skip, (name, i)
            else:
                assert na[i] == nb[i] and np.array_equal(la[i, : na[i]], lb[i, : nb[i]]), (name, i)


if __name__ == "__main__":
    _dump(sys.argv[1])
