"""The eager check step ``htfs_check_rebuild_nlist`` after it lost two of its nine stream operations: the displacement word filled
by ONE launch (``check_disp_kernel<T, false>``: work words in the list's scratch, a ticket, no memset) and the per-cell ordering
folded into ``bins_finish_kernel`` (out of place, from the scratch's staging words; it also zeroes the counts).

Every case runs the new call and the stepwise route -- ``htfs_max_displacement2`` into a zeroed word, the decision on the host,
``htfs_rebuild_nlist`` -- on the same inputs and asserts ``torch.equal`` on everything a check leaves behind; ``order`` is
compared with ``htfs_cell_index`` + ``htfs_cell_sort`` as well, which still sorts with ``cell_order_kernel``.  A neighbor row is
compared over its live entries (its tail is never written: ``test_gpu_standin.py`` has the same rule).

The status words keep their trailing copy: ``CellNlist`` polls them BEFORE it enqueues the next check
(``test_device_decided_rebuild_reports_row_overflow_late``), so they cannot ride in the next check's first kernel.  After a check
has completed the pinned words are that check's; after an open check k and a closed check k + 1 they are check k's, unchanged.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

R_LIST = 1.0
# (cells per axis, stencil half-width, box length): 27 cells at least r_list wide -- the walk per particle, one block of the scan;
# 4 096 cells at least r_list / 2 wide -- the walk per cell, two blocks of the scan
COARSE, FINE = (3, 1, 3.0), (16, 2, 8.0)


def test_scratch_word_count_of_the_header(tmp_path):
    """HTFS_SCRATCH_WORDS: counts + cursors + two work words + one staging word per binned position, no padding."""
    from helpers import ROOT
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "htf_standin.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu\\n", (size_t)HTFS_SCRATCH_WORDS(27, 1), (size_t)HTFS_SCRATCH_WORDS(1000, 1023),'
                   ' (size_t)HTFS_SCRATCH_WORDS(4096, 4097), (size_t)HTFS_SCRATCH_WORK(27), (size_t)HTFS_SCRATCH_STAGE(27)); return 0;}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [2 * 27 + 2 + 1, 2 * 1000 + 2 + 1023, 2 * 4096 + 2 + 4097, 54, 56]


class _List:
    """One htfs_nlist and every buffer behind it, filled with sentinels so that "untouched" can be told from "rewritten"."""

    def __init__(self, htf, dev, dtype, N, Ntot, grid, pitch, ref):
        n, sw, L = grid
        self.L, self.N, self.Ntot, self.pitch, self.ncell, self.dev = L, N, Ntot, pitch, n ** 3, dev
        self.code = htf._lib.HTF_F32 if dtype == torch.float32 else htf._lib.HTF_F64
        i32 = dict(dtype=torch.int32, device=dev)
        self.cell_of = torch.full((Ntot,), -7, **i32)
        # garbage everywhere: the first call passes scratch_clean = 0 and must zero what it needs zero
        self.scratch = torch.full((2 * self.ncell + 2 + Ntot,), 0x2B2B2B2B, **i32)
        self.cell_start = torch.full((self.ncell + 1,), -7, **i32)
        self.order = torch.full((Ntot,), -7, **i32)
        self.pos_sorted = torch.zeros((Ntot, 4), dtype=dtype, device=dev)
        self.ranges = torch.zeros(4 * self.ncell * (2 * sw + 1) ** 2, **i32)
        self.n_neigh = torch.full((N,), -7, **i32)
        self.head_list = torch.full((N,), -7, **i32)
        self.nlist = torch.full((N * pitch,), -7, **i32)
        self.stat = torch.zeros(2, **i32)             # [largest row, rebuilds]
        self.disp = torch.full((1,), 123.0, dtype=torch.float32, device=dev)   # (never zeroed by the host)
        self.ref = ref.clone()
        d = self.desc = htf._lib.Nlist()
        half = 0.5 * L
        d.box = htf._lib.make_box(np.array([[-half] * 3, [half] * 3, [0.0] * 3]), (1, 1, 1))
        d.r_list, d.pitch, d.type_split = R_LIST, pitch, -1
        d.ncell3[:] = [n] * 3
        d.stencil3[:] = [sw] * 3
        d.image_L[:] = [0.0] * 3
        for name in ("cell_of", "scratch", "cell_start", "order", "pos_sorted", "ranges", "n_neigh", "head_list", "nlist", "ref"):
            setattr(d, name, getattr(self, name).data_ptr())
        d.max_neigh, d.counter = self.stat.data_ptr(), self.stat.data_ptr() + 4

    def counts(self):
        return self.scratch[: self.ncell]

    def work(self):
        return self.scratch[2 * self.ncell: 2 * self.ncell + 2]

    def state(self):
        """Everything a check leaves behind ("Same bits"), the neighbor rows over their live entries."""
        torch.cuda.synchronize()
        live = torch.arange(self.pitch, device=self.dev)[None, :] < self.n_neigh[:, None]
        return dict(n_neigh=self.n_neigh.clone(), head_list=self.head_list.clone(), nlist=self.nlist.view(-1, self.pitch)[live].clone(),
                    cell_start=self.cell_start.clone(), order=self.order.clone(), pos_sorted=self.pos_sorted.clone(),
                    ref=self.ref.clone(), stat=self.stat.clone(), disp=self.disp.clone())


def _stream(htf, dev):
    from hoomd_tf_amd.ops import raw_stream
    return C.c_void_p(raw_stream(dev.index))


def _check_new(htf, l, pos, thr2, clean, h_stat=None):
    htf._lib.check(htf._lib.lib.htfs_check_rebuild_nlist(C.byref(l.desc), pos.data_ptr(), l.code, l.N, l.Ntot, int(clean), l.disp.data_ptr(),
                                                         float(thr2), l.stat.data_ptr(), None if h_stat is None else h_stat.data_ptr(),
                                                         _stream(htf, l.dev)))


def _word_ref(htf, l, pos):
    """The stepwise distance check: the largest d^2 as htfs_max_displacement2 leaves it in a zeroed word."""
    l.disp.zero_()
    htf._lib.check(htf._lib.lib.htfs_max_displacement2(pos.data_ptr(), l.ref.data_ptr(), l.code, l.N, C.byref(l.desc.box), l.disp.data_ptr(),
                                                       _stream(htf, l.dev)))
    return np.float32(l.disp.item())


def _check_ref(htf, l, pos, thr2):
    """The stepwise route: distance check, the gate's comparison (fp32, >) on the host, the whole rebuild."""
    word = _word_ref(htf, l, pos)
    if word > np.float32(thr2):
        htf._lib.check(htf._lib.lib.htfs_rebuild_nlist(C.byref(l.desc), pos.data_ptr(), l.code, l.N, l.Ntot, 0, _stream(htf, l.dev)))
    return word


def _order_by_cell_sort(htf, l, pos):
    """``order`` by the stepwise exports (cell_order_kernel), on buffers of its own."""
    i32 = dict(dtype=torch.int32, device=l.dev)
    cell_of, start, order = torch.empty(l.Ntot, **i32), torch.empty(l.ncell + 1, **i32), torch.full((l.Ntot,), -7, **i32)
    scratch = torch.empty(2 * l.ncell, **i32)
    s = _stream(htf, l.dev)
    htf._lib.check(htf._lib.lib.htfs_cell_index(pos.data_ptr(), l.code, l.Ntot, C.byref(l.desc.box), C.byref(l.desc.ncell3), cell_of.data_ptr(), s))
    htf._lib.check(htf._lib.lib.htfs_cell_sort(cell_of.data_ptr(), l.Ntot, l.ncell, scratch.data_ptr(), start.data_ptr(), order.data_ptr(), s))
    torch.cuda.synchronize()
    return start, order


def _same(a, b, what=""):
    for k in a:
        assert torch.equal(a[k], b[k]), "%s differs %s" % (k, what)


def _wrap(x, L):
    return x - np.round(x / L) * L


def _positions(rng, n, L, dtype, dev, step=0.05):
    """(ref, pos): n uniformly placed rows and the same rows moved by up to ``step`` per axis, both inside the box."""
    x0 = rng.uniform(-0.5 * L, 0.5 * L, (n, 3))
    x1 = _wrap(x0 + rng.uniform(-step, step, (n, 3)), L)
    mk = lambda x: torch.tensor(np.concatenate([x, np.zeros((n, 1))], axis=1), dtype=dtype, device=dev)  # noqa: E731
    return mk(x0), mk(x1)


def _pair(htf, dev, dtype, N, Ntot, grid, pitch, ref):
    return (_List(htf, dev, dtype, N, Ntot, grid, pitch, ref[:N]), _List(htf, dev, dtype, N, Ntot, grid, pitch, ref[:N]))


def _assert_clean(l):
    assert int(l.counts().abs().sum()) == 0 and int(l.work().abs().sum()) == 0, "counts or work words left dirty"


DTYPES = [torch.float32, torch.float64]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,grid,pitch", [(1, COARSE, 8), (1000, FINE, 64), (1025, FINE, 64), (4097, FINE, 128)],
                         ids=["n1", "n1000", "n1025", "n4097"])
def test_ticket_of_one_and_of_several_blocks(htf, cuda, dtype, N, grid, pitch):
    """N = 1 and 1000: the one block's ticket is the last; 1025: a second, nearly empty block; 4097: five."""
    rng = np.random.default_rng(N)
    ref, pos = _positions(rng, N, grid[2], dtype, cuda)
    new, old = _pair(htf, cuda, dtype, N, N, grid, pitch, ref)
    word = _check_ref(htf, old, pos, 0.0)
    assert word > 0
    _check_new(htf, new, pos, 0.0, clean=False)
    _same(new.state(), old.state())
    assert int(new.stat[1]) == 1 and int(new.stat[0]) <= pitch
    _assert_clean(new)
    start, order = _order_by_cell_sort(htf, new, pos)
    assert torch.equal(start, new.cell_start) and torch.equal(order, new.order)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_gate_just_closed_and_just_open(htf, cuda, dtype):
    """The threshold AT the reference's word holds the rebuild back (> , not >=) and nothing is touched; one ulp below opens it."""
    N, grid, pitch = 1025, FINE, 64
    rng = np.random.default_rng(3)
    ref, pos = _positions(rng, N, grid[2], dtype, cuda)
    new, old = _pair(htf, cuda, dtype, N, N, grid, pitch, ref)
    word = _word_ref(htf, old, pos)
    # closed
    new.scratch[: 2 * new.ncell + 2] = 0
    before = new.state()
    stage_before = new.scratch.clone()
    _check_new(htf, new, pos, float(word), clean=True)
    after = new.state()
    assert np.float32(after.pop("disp").item()) == word
    before.pop("disp")
    _same(after, before, "after a closed check")
    assert torch.equal(new.scratch, stage_before) and torch.equal(new.cell_of, torch.full_like(new.cell_of, -7))
    # open
    below = float(np.nextafter(word, np.float32(0.0)))
    assert _check_ref(htf, old, pos, below) == word
    _check_new(htf, new, pos, below, clean=True)
    _same(new.state(), old.state(), "after an open check")
    assert int(new.stat[1]) == 1
    _assert_clean(new)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_three_checks_on_one_list(htf, cuda, dtype):
    """Open, closed, open on one list with nothing re-zeroed from the host: work words and counts are left clean by every check."""
    N, grid, pitch = 4097, FINE, 128
    rng = np.random.default_rng(4)
    ref, pos1 = _positions(rng, N, grid[2], dtype, cuda)
    new, old = _pair(htf, cuda, dtype, N, N, grid, pitch, ref)
    move = lambda p, s: torch.cat([torch.tensor(_wrap(p[:, :3].cpu().numpy() + rng.uniform(-s, s, (N, 3)), grid[2]), dtype=dtype, device=cuda),  # noqa: E731
                                   p[:, 3:]], dim=1)
    pos2, thr = move(pos1, 0.01), 0.04   # (0.2^2: pos1 is up to 0.05 * sqrt(3) from ref, pos2 up to 0.01 * sqrt(3) from pos1)
    pos3 = move(pos2, 0.2)
    expect = []
    for k, (pos, clean) in enumerate(((pos1, False), (pos2, True), (pos3, True))):
        word = _check_ref(htf, old, pos, 0.0 if k == 0 else thr)
        _check_new(htf, new, pos, 0.0 if k == 0 else thr, clean=clean)
        _same(new.state(), old.state(), "after check %d" % k)
        _assert_clean(new)
        expect.append(bool(word > np.float32(0.0 if k == 0 else thr)))
    assert expect == [True, False, True] and int(new.stat[1]) == 2


def _crowded(rng, dtype, dev):
    """300 rows on the 27-cell grid: 100 in one cell, none in another, the indices DESCENDING in cell order (so the order the
    scatter's atomics arrive in is not the index order), ref = pos moved a little."""
    L = COARSE[2]
    x = rng.uniform(-0.5 * L, 0.5 * L, (200, 3))
    cell = lambda x: np.clip(np.floor((x + 0.5 * L) / L * 3), 0, 2).astype(int)  # noqa: E731
    x = x[~np.all(cell(x) == np.array([2, 1, 0]), axis=1)]                  # an empty cell
    crowd = rng.uniform(-0.5 * L + 0.01, -0.5 * L + 0.99, (300 - len(x), 3))   # cell (0, 0, 0)
    x = np.concatenate([x, crowd])
    c = cell(x)
    key = (c[:, 2] * 3 + c[:, 1]) * 3 + c[:, 0]
    x = x[np.argsort(-key, kind="stable")]
    assert len(x) == 300 and np.sum(key == 0) > 64 and not np.any(key == 5)
    x1 = _wrap(x + rng.uniform(-0.004, 0.004, x.shape), L)
    # keep every row in its cell (a move across a face would only change which cell is crowded, not what is tested)
    x1 = np.where(cell(x1) == cell(x), x1, x)
    mk = lambda a: torch.tensor(np.concatenate([a, np.zeros((300, 1))], axis=1), dtype=dtype, device=dev)  # noqa: E731
    return mk(x), mk(x1)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_a_cell_with_many_members_and_an_empty_one(htf, cuda, dtype):
    ref, pos = _crowded(np.random.default_rng(5), dtype, cuda)
    new, old = _pair(htf, cuda, dtype, 300, 300, COARSE, 304, ref)
    _check_ref(htf, old, pos, 0.0)
    _check_new(htf, new, pos, 0.0, clean=False)
    _same(new.state(), old.state())
    _assert_clean(new)
    start, order = _order_by_cell_sort(htf, new, pos)
    assert torch.equal(start, new.cell_start) and torch.equal(order, new.order)
    sizes = (new.cell_start[1:] - new.cell_start[:-1]).cpu().numpy()
    assert sizes.max() > 64 and sizes.min() == 0 and sizes.sum() == 300
    o = new.order.cpu().numpy()
    for c in range(27):   # ascending index inside every cell
        seg = o[int(new.cell_start[c]): int(new.cell_start[c + 1])]
        assert np.all(np.diff(seg) > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_ghost_candidates_behind_the_local_rows(htf, cuda, dtype):
    """Ntot > N: 1000 positions binned, 700 rows checked, searched and committed."""
    N, Ntot, grid, pitch = 700, 1000, FINE, 64
    ref, pos = _positions(np.random.default_rng(6), Ntot, grid[2], dtype, cuda)
    new, old = _pair(htf, cuda, dtype, N, Ntot, grid, pitch, ref)
    _check_ref(htf, old, pos, 0.0)
    _check_new(htf, new, pos, 0.0, clean=False)
    _same(new.state(), old.state())
    _assert_clean(new)
    assert int(new.cell_start[-1]) == Ntot and int(new.n_neigh.max()) > 0
    start, order = _order_by_cell_sort(htf, new, pos)
    assert torch.equal(start, new.cell_start) and torch.equal(order, new.order)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_inert_rows_in_the_middle(htf, cuda, dtype):
    """Rows whose x is NaN have not moved (d^2 = 0), are in no cell, and leave the tail of ``order`` and the sorted copy alone."""
    N, grid, pitch = 1025, FINE, 64
    ref, pos = _positions(np.random.default_rng(7), N, grid[2], dtype, cuda)
    pos[100:130, 0] = float("nan")
    ref[100:130, 0] = float("nan")
    pos[1024, 0] = float("nan")   # ... and the one row of the last block: its maximum is 0
    new, old = _pair(htf, cuda, dtype, N, N, grid, pitch, ref)
    word = _check_ref(htf, old, pos, 0.0)
    assert word > 0 and np.isfinite(word)
    _check_new(htf, new, pos, 0.0, clean=False)
    a, b = new.state(), old.state()
    # (bit patterns: the reference positions of the inert rows are NaN on both sides)
    for k in a:
        assert torch.equal(a[k].view(torch.uint8) if a[k].is_floating_point() else a[k],
                           b[k].view(torch.uint8) if b[k].is_floating_point() else b[k]), k
    _assert_clean(new)
    assert int(new.cell_start[-1]) == N - 31
    assert torch.equal(new.order[N - 31:], torch.full((31,), -7, dtype=torch.int32, device=cuda))
    assert torch.equal(new.cell_of[100:130], torch.full((30,), -1, dtype=torch.int32, device=cuda))   # kDeadCell: in no cell


@pytest.mark.gpu
def test_pinned_status_words(htf, cuda):
    """The pinned pair after a completed check is that check's [largest row, rebuilds]; a closed check leaves it as it was, so after
    an open check k and a closed check k + 1 the host still reads check k's words.  Never torn: both words come in one copy."""
    N, grid, pitch = 1000, FINE, 64
    rng = np.random.default_rng(8)
    ref, pos = _positions(rng, N, grid[2], torch.float32, cuda)
    new, _ = _pair(htf, cuda, torch.float32, N, N, grid, pitch, ref)
    h = torch.full((2,), -1, dtype=torch.int32).pin_memory()
    _check_new(htf, new, pos, 0.0, clean=False, h_stat=h)          # check k: open
    torch.cuda.synchronize()
    k_words = new.stat.cpu().clone()
    assert int(k_words[1]) == 1 and 0 < int(k_words[0]) <= pitch and torch.equal(h, k_words)
    _check_new(htf, new, pos, 1.0e6, clean=True, h_stat=h)         # check k + 1: closed
    torch.cuda.synchronize()
    assert torch.equal(h, k_words) and torch.equal(new.stat.cpu(), k_words)
    _, moved = _positions(rng, N, grid[2], torch.float32, cuda)
    _check_new(htf, new, moved, 0.0, clean=True, h_stat=h)         # check k + 2: open again
    torch.cuda.synchronize()
    assert int(new.stat[1]) == 2 and torch.equal(h, new.stat.cpu())
