"""The reference of the rebuild's products (tests/binning_ref.py) and its seeded cases, checked on the CPU alone: every case holds
the edge it stands for, and the reference's range table agrees with ``helpers.brute_nlist`` on which cells can hold a neighbor --
for every brute-force pair the neighbor's slot of the cell-sorted order is covered by exactly one run of the particle's cell, and
no slot is covered twice."""
import numpy as np
import pytest

import binning_ref as R
from helpers import brute_nlist

DTYPES = [np.float32, np.float64]
CROWDED = [c for c in R.CONFIGS]


@pytest.mark.parametrize("config", CROWDED)
def test_crowded_case_has_its_crowd_in_the_last_cell_and_descends(config):
    k = R.build_case(config, "crowded")
    b = k.expected(np.float64)
    sizes = np.diff(b.cell_start.astype(np.int64))
    assert sizes[-1] >= 200 and sizes[-1] == sizes.max(), "the crowded cell is the last one"
    assert sizes[0] == 0, "the first cell is empty"
    assert np.all(np.diff(b.cell_of.astype(np.int64)) <= 0), "indices descend in cell order"
    assert sizes.sum() == k.Ntot == b.live


@pytest.mark.parametrize("config", list(R.CONFIGS))
def test_ghost_case_has_inert_rows_at_the_ends(config):
    k = R.build_case(config, "ghosts")
    b = k.expected(np.float32)
    assert k.N < k.Ntot and abs(k.Ntot / k.N - 1.3) < 0.02
    for i in (0, k.N - 1, k.Ntot - 1):
        assert b.cell_of[i] == R.DEAD
    assert b.live == k.Ntot - int(np.isnan(k.xyz[:, 0]).sum()) < k.Ntot - 2
    assert int(b.cell_start[-1]) == b.live and len(b.order) == b.live
    assert not np.isin(b.ref_rows, [0, k.N - 1]).any() and len(b.ref_rows) < k.N
    assert np.any(b.order >= k.N), "ghosts are binned"


@pytest.mark.parametrize("config", list(R.CONFIGS))
def test_typed_case_has_both_sides_in_one_cell(config):
    k = R.build_case(config, "typed")
    b = k.expected(np.float64)
    assert k.type_split == 1 and set(np.unique(k.types)) == {0, 1, 2, 3}
    side = (b.sorted_tag >> 31) & 1
    assert np.array_equal(side, (k.types[b.order] >= 1).astype(np.int64))
    both = [c for c in range(k.ncell) if len(set(side[b.cell_start[c]: b.cell_start[c + 1]])) == 2]
    assert both, "no cell holds both sides of the split"
    assert np.array_equal(b.sorted_tag & (R.TAG_SIDE - 1), b.order)


@pytest.mark.parametrize("config", list(R.CONFIGS))
@pytest.mark.parametrize("population", R.POPULATIONS)
def test_cases_are_exact_in_both_precisions(config, population):
    """Same numbers, same cells, same rows whichever dtype stores them; nothing borderline; the grid sizes the issue names."""
    k = R.build_case(config, population)
    a = R.expected_bins(k.pos(np.float32), k.lo, k.hi, k.ncell3, k.stencil3, k.periodic, k.N, k.type_split, k.image_L, r_list=R.R_LIST)
    b = k.expected(np.float64)
    for name in ("cell_of", "cell_start", "order", "ranges", "n_neigh", "row_k"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(a.sorted_xyz.astype(np.float64), b.sorted_xyz) and a.sorted_xyz.dtype == np.float32
    x = a.binned_xyz[a.alive]
    for d in range(3):
        assert not R.borderline(x[:, d], k.lo[d], k.hi[d], k.ncell3[d], np.float32).any()
    assert np.array_equal(x * R.QUANTUM * 4, np.round(x * R.QUANTUM * 4)), "coordinates are multiples of 2^-12 at least"
    assert k.ncell == {"3x3x3": 27, "5x5x5": 125, "5x3x1": 15, "16x16x8": 2048, "17x11x11": 2057, "13x13x12": 2028,
                       "21x14x14": 4116}[R.CONFIGS[config][0]]
    assert a.max_neigh > 0 and k.Ntot <= 12500
    if any(k.image_L):
        stored = k.pos(np.float32)[:, 0].astype(np.float64)
        moved = np.abs(stored[a.alive] - a.binned_xyz[a.alive, 0])
        assert set(np.unique(moved)) == {0.0, 32.0} and abs((moved > 0).mean() - 0.1) < 0.02


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_planted_coordinates_land_in_the_cell_written_next_to_them(dtype):
    pos, want, lo, hi, n3 = R.planted_case(dtype)
    b = R.expected_bins(pos, lo, hi, n3, (2, 2, 2), (1, 1, 1), len(pos), -1, (0.0, 0.0, 0.0))
    assert np.array_equal(b.cell_of, want)
    assert (want == R.DEAD).sum() == 3 and len(np.unique(want)) > 60
    # the faces are there, bit for bit, hi included, and the last cell along every axis is reached by clamping
    for d in range(3):
        for f in range(n3[d] + 1):
            assert np.any(pos[:, d] == dtype(lo[d] + 0.5 * f))
        assert np.any(pos[:, d] > hi[d]) and np.any(pos[:, d] < lo[d])


def _helper_rows(k, b, rows):
    """``helpers.brute_nlist`` for the given rows (moved to the front: it takes the first n_local rows), indices mapped back."""
    rest = np.setdiff1d(np.arange(k.Ntot), rows)
    perm = np.concatenate([rows, rest])
    L = np.where(np.array(k.periodic) != 0, np.array(k.hi) - np.array(k.lo), 1.0e30)
    with np.errstate(invalid="ignore"):
        n_neigh, head, flat = brute_nlist(b.binned_xyz[perm], L, R.R_LIST, n_local=len(rows))
    i = np.repeat(rows, n_neigh.astype(np.int64))
    kk = perm[flat.astype(np.int64)]
    by_row = np.lexsort((kk, i))
    return i[by_row], kk[by_row]


def _runs(b, k):
    nrow = (2 * k.stencil3[1] + 1) * (2 * k.stencil3[2] + 1)
    u = R.unpack_ranges(b.ranges.reshape(k.ncell, nrow, 4))
    start = np.concatenate([u["start0"], u["start1"]], axis=1)
    length = np.concatenate([u["len0"], u["len1"]], axis=1)
    zero = np.zeros_like(u["code_x"])
    codes = np.stack([np.concatenate([zero, u["code_x"]], axis=1), np.concatenate([u["code_y"]] * 2, axis=1),
                      np.concatenate([u["code_z"]] * 2, axis=1)], axis=-1)
    return start, length, codes


@pytest.mark.parametrize("config", list(R.CONFIGS))
@pytest.mark.parametrize("population", R.POPULATIONS)
def test_runs_cover_every_brute_force_neighbor_exactly_once(config, population):
    k = R.build_case(config, population)
    b = k.expected(np.float64)
    start, length, codes = _runs(b, k)
    # no slot is covered twice: a cell's non-empty runs, sorted by their start, do not overlap
    big = np.int64(1) << 40
    st = np.where(length > 0, start, big)
    by = np.argsort(st, axis=1, kind="stable")
    st, en = np.take_along_axis(st, by, 1), np.take_along_axis(st + length, by, 1)
    assert np.all(st[:, 1:] >= en[:, :-1]), "two runs of a cell overlap"
    assert np.all(en <= np.where(st < big, b.live, big + b.live))
    # helpers.brute_nlist on the small cases' every row and on a sample of a large case's rows
    rng = np.random.default_rng(1)
    rows = np.arange(k.N) if k.Ntot <= 600 else np.sort(rng.choice(k.N, 384, replace=False))
    hi_, hk = _helper_rows(k, b, rows)
    if population != "typed":   # (the helper knows no type split: its pairs are a superset there)
        pick = np.isin(b.row_i, rows)
        assert np.array_equal(b.row_i[pick], hi_) and np.array_equal(b.row_k[pick], hk), "the chunked brute force disagrees with helpers.brute_nlist"
        pi, pk = b.row_i, b.row_k.astype(np.int64)    # all rows
    else:
        pi, pk = hi_, hk
    assert len(pi) > 0
    slot = np.full(k.Ntot, -1, dtype=np.int64)
    slot[b.order] = np.arange(b.live)
    shift_of = np.array([0.0, -1.0, 1.0])   # IMAGE_BELOW: seen a box length below
    L = np.array(k.hi) - np.array(k.lo)
    codes_bind = all(n >= 7 for n, p in zip(k.ncell3, k.periodic) if p)   # the search takes the image from the code on such grids
    for a in range(0, len(pi), 200000):
        i, kk = pi[a: a + 200000], pk[a: a + 200000]
        c, s = b.cell_of[i].astype(np.int64), slot[kk]
        assert np.all(s >= 0)
        inside = (start[c] <= s[:, None]) & (s[:, None] < start[c] + length[c])
        assert np.all(inside.sum(axis=1) == 1), "a neighbor's slot is not covered by exactly one run of the particle's cell"
        if codes_bind:
            run = np.argmax(inside, axis=1)
            d = b.binned_xyz[kk] + shift_of[codes[c, run]] * L - b.binned_xyz[i]
            assert np.all((d * d).sum(axis=1) <= R.R_LIST ** 2), "a run's image code is not the image the pair is a pair through"


def test_range_packing_round_trips():
    rng = np.random.default_rng(0)
    f = dict(start0=rng.integers(0, 1 << 31, 50), len0=rng.integers(0, 1 << 28, 50), code_y=rng.integers(0, 3, 50),
             code_z=rng.integers(0, 3, 50), start1=rng.integers(0, 1 << 31, 50), len1=rng.integers(0, 1 << 28, 50),
             code_x=rng.integers(0, 3, 50))
    t = R.pack_ranges(**f)
    assert t.dtype == np.uint32 and t.shape == (50, 4)
    for name, v in R.unpack_ranges(t).items():
        assert np.array_equal(v, f[name]), name
    # word 1 carries y in bits 28-29 and z in bits 30-31, word 3 carries x in bits 28-29
    one = R.pack_ranges(np.array([7]), np.array([5]), np.array([1]), np.array([2]), np.array([9]), np.array([3]), np.array([2]))[0]
    assert list(one) == [7, 5 | 1 << 28 | 2 << 30, 9, 3 | 2 << 28]


def test_non_periodic_rows_outside_the_grid_are_all_zero():
    k = R.build_case("3x3x3-nnn", "uniform")
    b = k.expected(np.float64)
    t = b.ranges.reshape(27, 9, 4)
    assert not t[0, 0].any() and not t[26, 8].any() and t[13].any(axis=1).all()   # corner cells' outward rows; the centre cell has all nine
    assert not t[..., 2:].any(), "no wrapped run on a non-periodic x"
    assert not (t[..., 1] >> R.RANGE_CODE_SHIFT).any(), "no image code on a non-periodic axis"


def test_sort_cases():
    seen = 0
    for ncell in R.SORT_NCELL:
        for Ntot in R.SORT_NTOT:
            for pattern in R.SORT_PATTERNS:
                c = R.sort_case(ncell, Ntot, pattern)
                if c is None:
                    assert pattern == "last" and Ntot > 300
                    continue
                seen += 1
                assert c.dtype == np.uint32 and len(c) == Ntot
                start, order = R.expected_sort(c, ncell)
                assert len(start) == ncell + 1 and start[-1] == len(order) == int((c != R.DEAD).sum())
                assert np.all(np.diff(c[order].astype(np.int64)) >= 0)
                if pattern == "dead" and Ntot:
                    assert c[0] == R.DEAD and c[-1] == R.DEAD
                if pattern == "descending":
                    assert np.all(np.diff(c.astype(np.int64)) <= 0)
                if pattern == "last":
                    assert np.all(c == ncell - 1)
    assert seen == 10 * 6 * 4 - 10


def test_classify_cases_reach_every_key_a_world_admits():
    for world, bounds in R.SLAB_BOUNDS.items():
        assert len(bounds) == world + 1
        seen = set()
        for dtype in DTYPES:
            for r_ghost in R.SLAB_R_GHOST:
                for bd in bounds:   # every threshold is a float32 number
                    for v in (bd, bd + r_ghost, bd - r_ghost):
                        assert float(np.float32(v)) == v
                for N in R.SLAB_N:
                    x = R.slab_positions(world, r_ghost, N, dtype)
                    assert len(x) == N and np.array_equal(x.astype(dtype).astype(np.float64), x)
                    if N >= 257:
                        for bd in bounds:
                            for v in (bd, bd + r_ghost, bd - r_ghost):
                                v = dtype(v)
                                for planted in (v, np.nextafter(v, dtype(100)), np.nextafter(v, dtype(-100))):
                                    assert np.any(x == float(planted))
                        assert np.any(x < -8.0) and np.any(x >= 8.0)
                    for rank in range(world):
                        seen |= set(R.expected_slab_keys(x, bounds, rank, r_ghost).tolist())
        assert seen == R.admitted_keys(world), (world, sorted(seen))
    # class 2 needs the wide ghost layer
    narrow = min(np.diff(R.SLAB_BOUNDS[3]))
    assert R.SLAB_R_GHOST[1] > narrow / 2 > R.SLAB_R_GHOST[0]


def test_segment_tables_have_empty_segments_first_middle_and_last():
    t = R.SEGMENT_TABLES
    assert t["three-first-empty"][0] == 0 and t["three-middle-empty"][1] == 0 and t["three-last-empty"][2] == 0
    s = t["sixteen"]
    assert len(s) == 16 and s[0] == 0 and s[-1] == 0 and 0 in s[1:-1] and s[3] == s[4] == 0
    assert sorted({len(v) for v in t.values()}) == [1, 3, 16] and not any(t["all-empty"]) and not any(t["sixteen-all-empty"])
    for name, counts in t.items():
        src_start, dst_start, cnt, rows_src, rows_dst = R.segment_case(counts)
        src = np.arange(rows_src * 3).reshape(rows_src, 3)
        dst = -np.ones((rows_dst, 3), dtype=np.int64)
        out = R.expected_segment_copy(dst, src, src_start, dst_start, cnt)
        assert (out >= 0).all(axis=1).sum() == sum(counts) and (out == -1).all(axis=1).sum() == rows_dst - sum(counts)


def test_key_cases():
    for N in R.KEY_N:
        for pattern in R.KEY_PATTERNS:
            key = R.key_case(N, pattern)
            start, order = R.expected_key_sort(key)
            assert len(key) == N and len(start) == 17 and start[16] == N and (key < 16).all()
            assert np.all(np.diff(key[order].astype(np.int64)) >= 0)
    assert set(R.key_case(257, "alternating")) == {0, 15} and set(R.key_case(64, "fifteens")) == {15}
