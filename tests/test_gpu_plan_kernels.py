"""The slab-plan kernels -- ``htfs_key_sort16`` (csrc/key_sort.h: tiles of 4 096, rounds of 256, waves of 64),
``htfs_slab_classify`` (the two-slab branch, the neighbors wrapped at rank 0 and rank world - 1) and ``htfs_segment_copy`` --
against the NumPy references of tests/binning_ref.py at the sizes where they take another path.  Integer results: exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import binning_ref as R

DTYPES = [torch.float32, torch.float64]
DTYPE_IDS = ["f32", "f64"]
NP = {torch.float32: np.float32, torch.float64: np.float64}
SENT = -7
GARBAGE = 0x2B2B2B2B


def _stream(dev):
    from hoomd_tf_amd.ops import raw_stream
    return C.c_void_p(raw_stream(dev.index))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("N", R.KEY_N)
def test_key_sort16(htf, cuda, N):
    """A stable argsort and the 17 starts, with N on either side of a wave, a round and a tile, from a scratch full of garbage."""
    lib, s = htf._lib, _stream(cuda)
    i32 = dict(dtype=torch.int32, device=cuda)
    for pattern in R.KEY_PATTERNS:
        key_np = R.key_case(N, pattern)
        want_start, want_order = R.expected_key_sort(key_np)
        key = torch.zeros(max(N, 1), **i32)
        key[:N] = torch.from_numpy(key_np.view(np.int32)).to(cuda)
        scratch = torch.full((max(16 * ((N + 4095) // 4096), 1),), GARBAGE, **i32)
        start = torch.full((17,), SENT, **i32)
        order = torch.full((N + 5,), SENT, **i32)
        lib.check(lib.lib.htfs_key_sort16(key.data_ptr(), N, scratch.data_ptr(), start.data_ptr(), order.data_ptr(), s))
        torch.cuda.synchronize()
        assert np.array_equal(_u32(start), want_start), (pattern, "starts")
        got = _u32(order)
        assert np.array_equal(got[:N], want_order), (pattern, "order")
        assert np.all(got[N:].view(np.int32) == SENT), (pattern, "order written behind N")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("world", sorted(R.SLAB_BOUNDS))
def test_slab_classify(htf, cuda, world, dtype):
    """key = destination * 4 + class for every rank of the world, positions planted on every bound and on bound +- r_ghost and one
    ulp either side of each, by the header's rules in float64 (every threshold is a float32 number: exact)."""
    lib, s = htf._lib, _stream(cuda)
    code = lib.HTF_F32 if dtype == torch.float32 else lib.HTF_F64
    bounds = R.SLAB_BOUNDS[world]
    bnd = torch.tensor(bounds, dtype=dtype, device=cuda)
    for r_ghost in R.SLAB_R_GHOST:
        for N in R.SLAB_N:
            x = R.slab_positions(world, r_ghost, N, NP[dtype])
            pos = torch.zeros((N, 4), dtype=dtype, device=cuda)
            pos[:, 0] = torch.from_numpy(x).to(cuda).to(dtype)
            pos[:, 1] = 1.0e9   # (y and z play no part)
            assert np.array_equal(pos[:, 0].cpu().numpy().astype(np.float64), x)
            for rank in range(world):
                key = torch.full((N + 3,), SENT, dtype=torch.int32, device=cuda)
                lib.check(lib.lib.htfs_slab_classify(pos.data_ptr(), code, N, bnd.data_ptr(), world, rank, float(r_ghost),
                                                     key.data_ptr(), s))
                torch.cuda.synchronize()
                got, want = _u32(key), R.expected_slab_keys(x, bounds, rank, r_ghost)
                bad = np.nonzero(got[:N] != want)[0]
                assert len(bad) == 0, (r_ghost, N, rank, [(float(x[i]), int(got[i]), int(want[i])) for i in bad[:5]])
                assert np.all(got[N:].view(np.int32) == SENT)


def _segment_copy(htf, cuda, counts, row_bytes, seed=0):
    lib, s = htf._lib, _stream(cuda)
    src_start, dst_start, cnt, rows_src, rows_dst = R.segment_case(counts, seed=seed)
    words = row_bytes // 4
    rng = np.random.default_rng([seed, row_bytes, len(counts)])
    src_np = rng.integers(0, 1 << 31, (rows_src, words)).astype(np.int32)
    dst_np = np.full((rows_dst, words), SENT, dtype=np.int32)
    src, dst = torch.from_numpy(src_np).to(cuda), torch.from_numpy(dst_np).to(cuda)
    as_c = lambda a: (C.c_uint * len(a))(*[int(v) for v in a])  # noqa: E731
    c_src, c_dst, c_cnt = as_c(src_start), as_c(dst_start), as_c(cnt)
    lib.check(lib.lib.htfs_segment_copy(dst.data_ptr(), src.data_ptr(), row_bytes, len(cnt), c_src, c_dst, c_cnt, s))
    torch.cuda.synchronize()
    want = R.expected_segment_copy(dst_np, src_np, src_start, dst_start, cnt)
    assert np.array_equal(dst.cpu().numpy(), want), (counts, row_bytes)
    assert np.array_equal(src.cpu().numpy(), src_np)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("row_bytes", R.SEGMENT_ROW_BYTES)
def test_segment_copy_tables(htf, cuda, row_bytes):
    """1, 3 and 16 segments with empty ones first, in the middle and last; rows no segment targets (a gap either side of each
    segment) keep their bits; all counts zero: nothing is touched."""
    for name, counts in R.SEGMENT_TABLES.items():
        want = _segment_copy(htf, cuda, counts, row_bytes)
        assert (want[:, 0] == SENT).sum() == len(want) - sum(counts), name


@pytest.mark.gpu
@pytest.mark.parametrize("counts,row_bytes", [((100, 0, 155), 4), ((100, 0, 156), 4), ((100, 0, 157), 4), ((85,), 12), ((0, 64, 0), 16),
                                              ((3, 5), 32), ((1000, 0, 1, 999), 32)],
                         ids=["255", "256", "257", "85x3", "64x4", "8x8", "2000x8"])
def test_segment_copy_around_a_block(htf, cuda, counts, row_bytes):
    """rows x words = 255, 256 and 257: the last block of the copy empty, full, and one word into the next."""
    _segment_copy(htf, cuda, counts, row_bytes, seed=1)
