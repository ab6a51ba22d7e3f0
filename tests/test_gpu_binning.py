"""The binning chain of a neighbor-list rebuild (csrc/standin.hip: cell_index_count_kernel, cell_scan_kernel, cell_scatter_kernel,
bins_finish_kernel, cell_ranges_body; and the stepwise exports cell_index_kernel, cell_count_kernel, cell_order_kernel,
gather4_kernel) against tests/binning_ref.py -- a NumPy restatement of the header's contracts -- product by product: ``cell_of``,
``cell_start``, ``order``, the tagged sorted copy, the range table, the reference positions, the status words and what the scratch
holds afterwards.  Everything is integer or bit-exact; the cases are built so that float32, float64 and the reference have one
answer (binning_ref's docstring says how), and tests/test_binning_ref_cpu.py checks the cases and the reference themselves.

The two routes -- ``htfs_rebuild_nlist`` and ``htfs_cell_index`` + ``htfs_cell_sort`` + ``htfs_gather4_tagged(_live)`` +
``htfs_build_nlist`` -- are each held against the reference, never against each other: they share the scan, the scatter and the
range table, and what is wrong in those is wrong on both sides.

The grids (r_list = 1):
  3x3x3 (stencil 1)      nx = 2 w + 1: the main and the wrapped run cover a row exactly once; also non-periodic
  5x5x5 (stencil 2)      the same for the fine stencil, too few cells for the image shift
  5x3x1 (2, 1, 0)        mixed stencils, a one-cell axis, nx != ny != nz; also periodic along x and z only
  16x16x8                2 048 cells: one full chunk of the scan; also with x re-imaged (image_L = 32)
  17x11x11               2 057: a second chunk of nine cells; also non-periodic
  13x13x12               2 028: a last chunk that is no multiple of eight
  21x14x14               4 116: a third chunk

What these tests were seen to catch, each as a one-line edit of a scratch copy of the library that moves no address: the side bit
dropped from the sorted copy's tag (the typed cases of the rebuild tests, test_gather4_tagged), the image codes 1 and 2 of the
wrapped x-run swapped (every rebuild case with a periodic x, on the range table), a cell's members ranked in descending order in
bins_finish_kernel and cell_order_kernel (test_cell_sort and every rebuild case, on ``order``).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import binning_ref as R

DTYPES = [torch.float32, torch.float64]
DTYPE_IDS = ["f32", "f64"]
NP = {torch.float32: np.float32, torch.float64: np.float64}
SENT = -7                      # integer buffers
SENT_BITS = 0x5A5A5A5A         # every 32-bit word of a Scalar4 buffer
GARBAGE = 0x2B2B2B2B           # the scratch on entry


def _stream(dev):
    from hoomd_tf_amd.ops import raw_stream
    return C.c_void_p(raw_stream(dev.index))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _scalar4(n, dtype, dev):
    """[n, 4] of ``dtype`` with every 32-bit word = SENT_BITS."""
    return torch.full((max(n, 1), 4 * (2 if dtype == torch.float64 else 1)), SENT_BITS, dtype=torch.int32, device=dev).view(dtype)


def _bits(a):
    return R.int_view(np.ascontiguousarray(a))


def _is_sentinel(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint32) == SENT_BITS))


def _code(htf, dtype):
    return htf._lib.HTF_F32 if dtype == torch.float32 else htf._lib.HTF_F64


class _Bins:
    """One htfs_nlist on any grid, stencil and periodicity, every buffer behind it filled with sentinels and the scratch with
    garbage, so that "not written" can be told from "written"."""

    def __init__(self, htf, dev, dtype, k, pitch, scratch=None):
        self.k, self.dev, self.dtype, self.pitch = k, dev, dtype, pitch
        self.N, self.Ntot, self.ncell = k.N, k.Ntot, k.ncell
        self.code = _code(htf, dtype)
        self.nrow = (2 * k.stencil3[1] + 1) * (2 * k.stencil3[2] + 1)
        i32 = dict(dtype=torch.int32, device=dev)
        words = 2 * self.ncell + 2 + self.Ntot
        if scratch is None:
            scratch = torch.full((words,), GARBAGE, **i32)
        assert scratch.numel() >= words and scratch.data_ptr() % 16 == 0
        self.scratch = scratch
        self.cell_of = torch.full((self.Ntot,), SENT, **i32)
        self.cell_start = torch.full((self.ncell + 1,), SENT, **i32)
        self.order = torch.full((self.Ntot,), SENT, **i32)
        self.pos_sorted = _scalar4(self.Ntot, dtype, dev)
        self.ranges = torch.full((4 * self.ncell * self.nrow,), SENT, **i32)
        self.n_neigh = torch.full((self.N,), SENT, **i32)
        self.head_list = torch.full((self.N,), SENT, **i32)
        self.nlist = torch.full((self.N * pitch,), SENT, **i32)
        self.stat = torch.tensor([0x7777, 41], **i32)   # [largest row, rebuilds]
        self.ref = _scalar4(self.N, dtype, dev)
        d = self.desc = htf._lib.Nlist()
        d.box = htf._lib.make_box(np.array([k.lo, k.hi, [0.0] * 3]), tuple(k.periodic))
        d.r_list, d.pitch, d.type_split = R.R_LIST, pitch, k.type_split
        d.ncell3[:] = list(k.ncell3)
        d.stencil3[:] = list(k.stencil3)
        d.image_L[:] = list(k.image_L)
        for name in ("cell_of", "scratch", "cell_start", "order", "pos_sorted", "ranges", "n_neigh", "head_list", "nlist", "ref"):
            setattr(d, name, getattr(self, name).data_ptr())
        d.max_neigh, d.counter = self.stat.data_ptr(), self.stat.data_ptr() + 4
        self.pos = torch.from_numpy(k.pos(NP[dtype])).to(dev)


def _rebuild(htf, l, clean=0):
    lib = htf._lib
    lib.check(lib.lib.htfs_rebuild_nlist(C.byref(l.desc), l.pos.data_ptr(), l.code, l.N, l.Ntot, int(clean), _stream(l.dev)))


def _stepwise(htf, l, inert):
    lib, s, d = htf._lib, _stream(l.dev), l.desc
    lib.check(lib.lib.htfs_cell_index(l.pos.data_ptr(), l.code, l.Ntot, C.byref(d.box), C.byref(d.ncell3), l.cell_of.data_ptr(), s))
    lib.check(lib.lib.htfs_cell_sort(l.cell_of.data_ptr(), l.Ntot, l.ncell, l.scratch.data_ptr(), l.cell_start.data_ptr(),
                                     l.order.data_ptr(), s))
    if inert:   # only the binned rows have an entry: their number is the last word of cell_start, read on the device
        lib.check(lib.lib.htfs_gather4_tagged_live(l.pos_sorted.data_ptr(), l.pos.data_ptr(), l.order.data_ptr(), l.code, l.Ntot,
                                                   l.cell_start.data_ptr() + 4 * l.ncell, d.type_split, s))
    else:
        lib.check(lib.lib.htfs_gather4_tagged(l.pos_sorted.data_ptr(), l.pos.data_ptr(), l.order.data_ptr(), l.code, l.Ntot,
                                              d.type_split, s))
    lib.check(lib.lib.htfs_build_nlist(C.byref(d), l.pos.data_ptr(), l.code, l.N, s))


def _assert_products(l, e, one_call, rows):
    """Every product of a rebuild against the reference ``e``; ``rows``: also the neighbor rows, as sets."""
    torch.cuda.synchronize()
    k, live, N = l.k, e.live, l.N
    assert np.array_equal(_u32(l.cell_of), e.cell_of), "cell_of"
    assert np.array_equal(_u32(l.cell_start), e.cell_start), "cell_start"
    order = _u32(l.order)
    assert np.array_equal(order[:live], e.order), "order (ascending index inside a cell)"
    assert np.all(order[live:].view(np.int32) == SENT), "order behind the binned total was written"
    ps = l.pos_sorted.cpu().numpy()[: l.Ntot]
    assert np.array_equal(_bits(ps[:live, :3]), _bits(e.sorted_xyz)), "pos_sorted x, y, z"
    tag = _bits(ps[:live, 3:])[:, 0].astype(np.int64) & (0xFFFFFFFF if l.dtype == torch.float32 else -1)
    assert np.array_equal(tag & (R.TAG_SIDE - 1), e.order), "pos_sorted w: the index"
    assert np.array_equal(tag, e.sorted_tag), "pos_sorted w: the side bit"
    assert np.array_equal(_u32(l.ranges).reshape(-1, 4), e.ranges), "ranges"
    # status and rows
    stat = l.stat.cpu().numpy()
    assert int(stat[0]) == e.max_neigh, "max_neigh: the largest true row count"
    # (an inert row's words are not compared: the walk per particle writes it an empty row, the walk per cell never visits a row
    # that is in no cell and leaves n_neigh and head_list as they were -- htfs_brick_migrate_merge zeroes those itself -- and the
    # header promises neither)
    has_row = e.alive[:N]
    n_neigh = np.where(has_row, _u32(l.n_neigh), 0)
    assert np.array_equal(n_neigh, e.n_neigh), "n_neigh"
    assert np.array_equal(_u32(l.head_list)[has_row], (np.arange(N, dtype=np.uint32) * l.pitch)[has_row]), "head_list"
    if rows:
        nl = _u32(l.nlist).reshape(N, l.pitch).copy()
        valid = np.arange(l.pitch)[None, :] < n_neigh[:, None]
        nl[~valid] = 0xFFFFFFFF
        nl.sort(axis=1)
        assert np.array_equal(nl[valid], e.row_k), "neighbor rows differ from brute force"
    counts = _u32(l.scratch[: l.ncell])
    assert not counts.any(), "the per-cell counts are not left zero"
    ref = l.ref.cpu().numpy()[:N]
    if one_call:
        pos = l.pos.cpu().numpy()
        assert np.array_equal(_bits(ref[e.ref_rows]), _bits(pos[e.ref_rows])), "ref"
        assert int(stat[1]) == 42, "counter"
        assert not _u32(l.scratch[2 * l.ncell: 2 * l.ncell + 2]).any(), "the work words are not left zero"
        # the staging words: a permutation of the binned indices, every cell's members inside that cell's span, in any order
        stage = _u32(l.scratch[2 * l.ncell + 2: 2 * l.ncell + 2 + live])
        assert np.array_equal(np.sort(stage), np.sort(e.order)), "staging words"
        assert np.array_equal(e.cell_of[stage], e.slot_cell), "a staging word outside its cell's span"
    else:
        assert _is_sentinel(ref) and int(stat[1]) == 41, "the stepwise route commits nothing"


# ---------------------------------------------------------------------------- (a) htfs_cell_sort on synthetic cell indices
@pytest.mark.gpu
@pytest.mark.parametrize("pattern", R.SORT_PATTERNS)
@pytest.mark.parametrize("ncell", R.SORT_NCELL)
def test_cell_sort(htf, cuda, ncell, pattern):
    """cell_count / cell_scan / cell_scatter / cell_order on cell counts around the scan's chunk (2 048) and its eight cells per
    thread, and particle counts around a block: cell_start, order[:live], an untouched tail, zero counts afterwards."""
    i32 = dict(dtype=torch.int32, device=cuda)
    lib, s = htf._lib, _stream(cuda)
    ran = 0
    for Ntot in R.SORT_NTOT:
        c = R.sort_case(ncell, Ntot, pattern)
        if c is None:
            continue
        ran += 1
        want_start, want_order = R.expected_sort(c, ncell)
        cell_of = torch.zeros(max(Ntot, 1), **i32)
        cell_of[:Ntot] = torch.from_numpy(c.view(np.int32)).to(cuda)
        scratch = torch.full((2 * ncell,), GARBAGE, **i32)
        start = torch.full((ncell + 1,), SENT, **i32)
        order = torch.full((max(Ntot, 1),), SENT, **i32)   # (at least one element: a null pointer is refused)
        lib.check(lib.lib.htfs_cell_sort(cell_of.data_ptr(), Ntot, ncell, scratch.data_ptr(), start.data_ptr(), order.data_ptr(), s))
        torch.cuda.synchronize()
        live = len(want_order)
        assert np.array_equal(_u32(start), want_start), (Ntot, "cell_start")
        got = _u32(order)
        assert np.array_equal(got[:live], want_order), (Ntot, "order")
        assert np.all(got[live:].view(np.int32) == SENT), (Ntot, "tail of order")
        assert not _u32(scratch[:ncell]).any(), (Ntot, "counts")
    assert ran >= 3


# ---------------------------------------------------------------------------- (b) htfs_cell_index
def _cell_index(htf, cuda, pos_np, lo, hi, ncell3, dtype):
    lib = htf._lib
    pos = torch.from_numpy(pos_np).to(cuda)
    box = lib.make_box(np.array([lo, hi, [0.0] * 3]), (1, 1, 1))
    n3 = (C.c_int * 3)(*ncell3)
    cell_of = torch.full((len(pos_np) + 3,), SENT, dtype=torch.int32, device=cuda)
    lib.check(lib.lib.htfs_cell_index(pos.data_ptr(), _code(htf, dtype), len(pos_np), C.byref(box), C.byref(n3), cell_of.data_ptr(),
                                      _stream(cuda)))
    torch.cuda.synchronize()
    got = _u32(cell_of)
    assert np.all(got[len(pos_np):].view(np.int32) == SENT)
    return got[: len(pos_np)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_cell_index_planted(htf, cuda, dtype):
    """Every face of a power-of-two box exactly, hi itself, one ulp either side, outside the box, NaN in x: the cell written next
    to each coordinate by hand (x fastest)."""
    pos, want, lo, hi, n3 = R.planted_case(NP[dtype])
    got = _cell_index(htf, cuda, pos, lo, hi, n3, dtype)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(pos[i, :3].tolist(), int(got[i]), int(want[i])) for i in bad[:5]]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("grid", list(R.GRIDS))
def test_cell_index_uniform(htf, cuda, grid, dtype):
    """nx != ny != nz with x fastest, boxes whose 1 / L is inexact, inert rows."""
    for population in ("uniform", "ghosts"):
        k = R.build_case(grid + "-ppp", population)
        got = _cell_index(htf, cuda, k.pos(NP[dtype]), k.lo, k.hi, k.ncell3, dtype)
        assert np.array_equal(got, k.expected(NP[dtype]).cell_of), population


# ---------------------------------------------------------------------------- (c) htfs_gather4_tagged(_live)
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_gather4_tagged(htf, cuda, n, dtype):
    """dest[i] = src[order[i]] with x, y, z bit for bit and w = order[i] | (type >= type_split) << 31, read as an integer of the
    scalar's width; with a live count on the device the rows behind it keep their bits."""
    lib, s, code = htf._lib, _stream(cuda), _code(htf, dtype)
    rng = np.random.default_rng([n, code])
    types = rng.integers(0, 4, n).astype(np.int32)
    types[: min(n, 4)] = np.arange(4)[: min(n, 4)]
    src_np = R.make_pos(rng.standard_normal((n, 3)) * 100.0, types, NP[dtype])
    src_np[0, 1] = np.nan            # (bits travel, whatever they mean)
    order_np = rng.permutation(n).astype(np.int32)
    src, order = torch.from_numpy(src_np).to(cuda), torch.from_numpy(order_np).to(cuda)
    n_live_dev = torch.zeros(1, dtype=torch.int32, device=cuda)
    mask = 0xFFFFFFFF if dtype == torch.float32 else -1
    for split in (-1, 0, 2):
        side = (types[order_np] >= split).astype(np.int64) if split >= 0 else np.zeros(n, np.int64)
        want_tag = order_np.astype(np.int64) | (side << 31)
        for n_live in [None] + sorted({0, 1, n - 1, n}):
            dest = _scalar4(n, dtype, cuda)
            if n_live is None:
                lib.check(lib.lib.htfs_gather4_tagged(dest.data_ptr(), src.data_ptr(), order.data_ptr(), code, n, split, s))
                m = n
            else:
                n_live_dev.fill_(n_live)
                lib.check(lib.lib.htfs_gather4_tagged_live(dest.data_ptr(), src.data_ptr(), order.data_ptr(), code, n,
                                                           n_live_dev.data_ptr(), split, s))
                m = n_live
            torch.cuda.synchronize()
            got = dest.cpu().numpy()[:n]
            assert np.array_equal(_bits(got[:m, :3]), _bits(src_np[order_np[:m], :3])), (split, n_live, "x, y, z")
            assert np.array_equal(_bits(got[:m, 3:])[:, 0].astype(np.int64) & mask, want_tag[:m]), (split, n_live, "tag")
            assert _is_sentinel(got[m:]), (split, n_live, "rows behind the live count were written")


# ---------------------------------------------------------------------------- (d) the whole rebuild, each product by itself
def _pitch(e):
    return e.max_neigh + 8


REBUILD_CASES = [(c, p) for c in R.CONFIGS for p in R.POPULATIONS]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("config,population", REBUILD_CASES, ids=["%s-%s" % cp for cp in REBUILD_CASES])
def test_rebuild_products(htf, cuda, config, population, dtype):
    """htfs_rebuild_nlist: five launches, every product against the reference (the rows in float64, as sets)."""
    k = R.build_case(config, population)
    e = k.expected(NP[dtype])
    l = _Bins(htf, cuda, dtype, k, _pitch(e))
    _rebuild(htf, l, clean=0)
    _assert_products(l, e, one_call=True, rows=dtype == torch.float64)


STEPWISE_CASES = [(c, p) for c, p in REBUILD_CASES if not any(R.CONFIGS[c][2])]   # (the stepwise exports know no image_L)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("config,population", STEPWISE_CASES, ids=["%s-%s" % cp for cp in STEPWISE_CASES])
def test_stepwise_products(htf, cuda, config, population, dtype):
    """htfs_cell_index + htfs_cell_sort + htfs_gather4_tagged(_live) + htfs_build_nlist against the same reference."""
    k = R.build_case(config, population)
    e = k.expected(NP[dtype])
    l = _Bins(htf, cuda, dtype, k, _pitch(e))
    _stepwise(htf, l, inert=e.live < k.Ntot)
    _assert_products(l, e, one_call=False, rows=dtype == torch.float64)
    ps = l.pos_sorted.cpu().numpy()[: k.Ntot]
    assert _is_sentinel(ps[e.live:]), "the sorted copy behind the binned total was written"


# ---------------------------------------------------------------------------- (e) one scratch across grids
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_one_scratch_across_grids(htf, cuda, dtype):
    """2 057 cells, then 27, then 2 057 again on ONE scratch with scratch_clean = 0: the small grid's cursors, work words and
    staging words lie where the large grid keeps its counts, and each rebuild must zero what it needs zero.  A fourth rebuild on
    the same grid as the third may then pass scratch_clean = 1."""
    seq = [("17x11x11-ppp", "uniform", 0), ("3x3x3-ppp", "crowded", 0), ("17x11x11-ppp", "ghosts", 0), ("17x11x11-ppp", "typed", 1)]
    cases = [R.build_case(c, p) for c, p, _ in seq]
    words = max(2 * k.ncell + 2 + k.Ntot for k in cases)
    scratch = torch.full((words,), GARBAGE, dtype=torch.int32, device=cuda)
    for k, (_, _, clean) in zip(cases, seq):
        e = k.expected(NP[dtype])
        l = _Bins(htf, cuda, dtype, k, _pitch(e), scratch=scratch)
        _rebuild(htf, l, clean=clean)
        _assert_products(l, e, one_call=True, rows=dtype == torch.float64)
