// Frame selection by committee deviation on the device (include/htf_select.h, htf.DeviationSelector): one update is three
// launches on the caller's stream and nothing the host waits for.
//
//   reduce   grid-stride blocks of 256 over the strided column of d_dev [N][2]; each leaves one (value, index) pair
//   decide   one block: the pair of the partials, the class, the counters, the slot (for "largest" a scan of the stored s)
//   store    one 16- or 32-byte row of d_pos per lane to the slot's frame, the box in block 0; returns at slot -1
//
// The launches hand over through global memory at kernel boundaries of one stream: no fences, no atomics, no polling.  The
// decision is made by one thread of the single decide block with plain stores.  The pair (s, a) is the greatest element of a
// total order (sel_greater), so lanes, waves, blocks and partials may be combined in any order: every grid gives the same bits.
#include "htf_select.h"
#include "htf_common.h"

#include <cmath>
#include <cstdint>

namespace htf {
namespace {

constexpr int kSelThreads = 256;
constexpr int kSelWaves = kSelThreads / 64;
constexpr unsigned kSelStoreBlocks = 2048;   // the copy's grid cap: eight blocks per compute unit, the rest by stride

struct SelPair {
    float v;
    unsigned i;
};

// below every pair a real row can form: -inf at an index no row has (N <= 2^32 - 1, so i <= 2^32 - 2)
__device__ __forceinline__ SelPair sel_lowest() { return SelPair{-INFINITY, 0xFFFFFFFFu}; }

// The greater of two pairs: NaN above every number, larger values above smaller ones, the lower index at equal values (and among
// NaNs).  Two pairs of different rows are never equal in this order, so the result of any combination tree is the same pair.
__device__ __forceinline__ SelPair sel_greater(SelPair p, SelPair q) {
    const bool pn = p.v != p.v, qn = q.v != q.v;
    const bool take_p = (pn || qn) ? (pn && (!qn || p.i < q.i)) : (p.v > q.v || (p.v == q.v && p.i < q.i));
    return take_p ? p : q;
}

// the greatest pair of the block, in every thread; s_part is reusable on return
__device__ __forceinline__ SelPair sel_block_greatest(SelPair p, SelPair *s_part) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        SelPair q;
        q.v = __shfl_xor(p.v, m);
        q.i = (unsigned)__shfl_xor((int)p.i, m);
        p = sel_greater(p, q);
    }
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = p;
    __syncthreads();
    p = s_part[0];
#pragma unroll
    for (int w = 1; w < kSelWaves; ++w) p = sel_greater(p, s_part[w]);
    __syncthreads();
    return p;
}

__global__ __launch_bounds__(kSelThreads) void sel_reduce_kernel(const float *__restrict__ dev, unsigned N, int column,
                                                                 unsigned *__restrict__ partials) {
    __shared__ SelPair s_part[kSelWaves];
    SelPair p = sel_lowest();
    const size_t stride = (size_t)gridDim.x * kSelThreads;
    for (size_t i = (size_t)blockIdx.x * kSelThreads + threadIdx.x; i < N; i += stride)
        p = sel_greater(p, SelPair{dev[2 * i + column], (unsigned)i});
    p = sel_block_greatest(p, s_part);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = __float_as_uint(p.v);
        partials[2 * blockIdx.x + 1] = p.i;
    }
}

__global__ __launch_bounds__(kSelThreads) void sel_decide_kernel(unsigned *__restrict__ state, unsigned capacity, unsigned n_parts,
                                                                 float lo, float hi, int policy) {
    __shared__ SelPair s_part[kSelWaves];
    float *slot_s = reinterpret_cast<float *>(state + HTF_SEL_HEADER_WORDS);
    unsigned *slot_a = state + HTF_SEL_HEADER_WORDS + capacity, *slot_stamp = slot_a + capacity;
    const unsigned *partials = slot_stamp + capacity;
    const unsigned stored = state[HTF_SEL_STORED];   // (thread 0 writes it behind the barriers of the two reductions)

    SelPair p = sel_lowest();
    for (unsigned j = threadIdx.x; j < n_parts; j += kSelThreads)
        p = sel_greater(p, SelPair{__uint_as_float(partials[2 * j]), partials[2 * j + 1]});
    p = sel_block_greatest(p, s_part);

    // the lowest slot holding the smallest stored s, as the greatest (-s, slot): a stored s is never NaN, and negation is exact
    SelPair m = sel_lowest();
    if (policy == HTF_SEL_LARGEST && stored >= capacity)
        for (unsigned j = threadIdx.x; j < capacity; j += kSelThreads) m = sel_greater(m, SelPair{-slot_s[j], j});
    m = sel_block_greatest(m, s_part);

    if (threadIdx.x != 0) return;
    const float s = p.v;
    const unsigned stamp = state[HTF_SEL_SEEN];
    state[HTF_SEL_SEEN] = stamp + 1;
    int slot = -1;
    if (s != s || (hi < INFINITY && s >= hi)) {
        state[HTF_SEL_FAILED] += 1;
    } else if (s < lo) {
        state[HTF_SEL_ACCURATE] += 1;
    } else {
        state[HTF_SEL_CANDIDATE] += 1;
        if (stored < capacity) {
            slot = (int)stored;
            state[HTF_SEL_STORED] = stored + 1;
        } else if (policy == HTF_SEL_LARGEST && s > -m.v) {
            slot = (int)m.i;
            state[HTF_SEL_REPLACED] += 1;
        } else {
            state[HTF_SEL_DROPPED] += 1;
        }
    }
    state[HTF_SEL_SLOT] = (unsigned)slot;
    state[HTF_SEL_LAST] = __float_as_uint(s);
    state[HTF_SEL_LAST + 1] = __float_as_uint((float)p.i);
    if (slot >= 0) {
        slot_s[slot] = s;
        slot_a[slot] = p.i;
        slot_stamp[slot] = stamp;
    }
}

template <typename T>
__global__ __launch_bounds__(kSelThreads) void sel_store_kernel(const unsigned *__restrict__ state, unsigned capacity,
                                                                const typename Vec4<T>::type *__restrict__ pos,
                                                                const T *__restrict__ box, unsigned N,
                                                                typename Vec4<T>::type *__restrict__ frames, T *__restrict__ boxes) {
    const unsigned slot = state[HTF_SEL_SLOT];
    if (slot >= capacity) return;   // -1: nothing to store (and no word a caller wrote there can send the copy out of the buffer)
    typename Vec4<T>::type *dst = frames + (size_t)slot * N;
    const size_t stride = (size_t)gridDim.x * kSelThreads;
    for (size_t i = (size_t)blockIdx.x * kSelThreads + threadIdx.x; i < N; i += stride) dst[i] = pos[i];
    if (blockIdx.x == 0 && threadIdx.x < 9) boxes[(size_t)slot * 9 + threadIdx.x] = box ? box[threadIdx.x] : T(0);
}

template <typename T>
void sel_launch_store(const unsigned *state, unsigned capacity, const void *pos, const void *box, unsigned N, void *frames, void *boxes,
                      hipStream_t stream) {
    using V = typename Vec4<T>::type;
    const unsigned rows = (N + kSelThreads - 1) / kSelThreads;
    hipLaunchKernelGGL((sel_store_kernel<T>), dim3(rows < kSelStoreBlocks ? rows : kSelStoreBlocks), dim3(kSelThreads), 0, stream, state,
                       capacity, (const V *)pos, (const T *)box, N, (V *)frames, (T *)boxes);
}

} // namespace
} // namespace htf

using namespace htf;

extern "C" unsigned long long htf_sel_state_words(unsigned capacity) {
    if (capacity < 1 || capacity > HTF_SEL_MAX_CAPACITY) return 0;
    return (unsigned long long)HTF_SEL_HEADER_WORDS + 3ull * capacity + 2ull * HTF_SEL_MAX_BLOCKS;
}

extern "C" int htf_sel_update(const float *d_dev, unsigned N, int column, float lo, float hi, int policy, unsigned capacity,
                              unsigned *d_state, const void *d_pos, const void *d_box, int dtype, void *d_frames, void *d_boxes,
                              unsigned max_blocks, htf_stream stream) {
    HTF_REQUIRE(d_dev && d_state && d_pos && d_frames && d_boxes, "htf_sel_update: null pointer");
    HTF_REQUIRE(capacity >= 1 && capacity <= HTF_SEL_MAX_CAPACITY, "htf_sel_update: capacity %u outside [1, %u]", capacity,
                HTF_SEL_MAX_CAPACITY);
    HTF_REQUIRE(N >= 1, "htf_sel_update: N must be >= 1");
    HTF_REQUIRE(dtype == HTF_F32 || dtype == HTF_F64, "htf_sel_update: bad dtype %d", dtype);
    HTF_REQUIRE(policy == HTF_SEL_FIRST || policy == HTF_SEL_LARGEST, "htf_sel_update: bad policy %d", policy);
    HTF_REQUIRE(column == HTF_SEL_FORCE || column == HTF_SEL_ENERGY, "htf_sel_update: bad column %d", column);
    HTF_REQUIRE(std::isfinite(lo) && lo >= 0.0f && lo <= hi, "htf_sel_update: thresholds must be 0 <= lo <= hi with lo finite (lo %g, hi %g)",
                (double)lo, (double)hi);
    HTF_REQUIRE(max_blocks <= HTF_SEL_MAX_BLOCKS, "htf_sel_update: max_blocks %u above %u", max_blocks, HTF_SEL_MAX_BLOCKS);
    HTF_REQUIRE((reinterpret_cast<uintptr_t>(d_pos) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_frames) & 15) == 0,
                "htf_sel_update: positions and frame buffer must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const unsigned cap = max_blocks ? max_blocks : HTF_SEL_MAX_BLOCKS;
    const unsigned rows = (N + kSelThreads - 1) / kSelThreads;
    const unsigned n_parts = rows < cap ? rows : cap;
    unsigned *partials = d_state + HTF_SEL_HEADER_WORDS + 3 * (size_t)capacity;
    hipLaunchKernelGGL(sel_reduce_kernel, dim3(n_parts), dim3(kSelThreads), 0, st, d_dev, N, column, partials);
    int rc = check_launch("sel_reduce_kernel");
    if (rc != HTF_OK) return rc;
    hipLaunchKernelGGL(sel_decide_kernel, dim3(1), dim3(kSelThreads), 0, st, d_state, capacity, n_parts, lo, hi, policy);
    rc = check_launch("sel_decide_kernel");
    if (rc != HTF_OK) return rc;
    if (dtype == HTF_F32)
        sel_launch_store<float>(d_state, capacity, d_pos, d_box, N, d_frames, d_boxes, st);
    else
        sel_launch_store<double>(d_state, capacity, d_pos, d_box, N, d_frames, d_boxes, st);
    return check_launch("sel_store_kernel");
}

extern "C" int htf_sel_reset(unsigned *d_state, unsigned capacity, htf_stream stream) {
    HTF_REQUIRE(d_state, "htf_sel_reset: null pointer");
    HTF_REQUIRE(capacity >= 1 && capacity <= HTF_SEL_MAX_CAPACITY, "htf_sel_reset: capacity %u outside [1, %u]", capacity,
                HTF_SEL_MAX_CAPACITY);
    HTF_CHECK_HIP(hipMemsetAsync(d_state, 0, (size_t)htf_sel_state_words(capacity) * sizeof(unsigned), (hipStream_t)stream));
    return HTF_OK;
}
