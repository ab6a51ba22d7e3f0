// The cell-binned route of compute_nlist (include/htf_nlist.h): the list htf_cg_nlist_forward (cg_map.hip) builds, bit for
// bit, from the particles of each row's 27 neighboring cells instead of all M.
//
// Built with -ffp-contract=off (Makefile), like cg_map.hip: distances, keys and the insertion step are nlist_select.h's,
// applied to the raw fp32 positions.  Since a row's list is the NN smallest keys it was offered, in any order, a search
// that offers every pair at d <= r_cut (and possibly more) returns what the all-pairs search returns.
//
// Why every such pair is offered.  Per dimension (L = L_c, u = 2^-24, r = r_cut), pair_of forms
//   D = fl(x_j - x_i),  k = rint(fl(D / L)),  dx = fl(D - fl(k L)),
// so dx = [(x_j - x_i) - k L + (x_j - x_i) e1 - k L e2] (1 + e3) with |e| <= u, and the exact periodic image
// E = (x_j - x_i) - k L obeys |E| <= |dx| (1 + 2u) + u |x_j - x_i| + u |k L|.  The binned particles have |x| <= 64 L, so
// |x_j - x_i| <= 128 L and |k| <= 129: |E| <= |dx| (1 + 2u) + 257 u L.  A kept pair has d <= r and, the sum of squares and
// sqrt being correctly rounded and monotone, |dx| <= r (1 + 2u).  So the exact distance between the two wrapped
// coordinates, measured round the period, is below r + 5 u r + 257 u L < r + 2^-14 (L + r) <= the cell width the caller
// chose: the two cells differ by at most one along every dimension (with n_c >= 3 the 27 stencil cells are distinct).
// The binning wraps in fp64 (|x / L| <= 64: the cell boundaries move by less than 2^-46 L), far inside the margin.
// Particles outside that range, or not finite, go into one extra cell that every row searches, and search all M themselves.
#include "htf_common.h"
#include "htf_nlist.h"
#include "htf_standin.h"
#include "nlist_select.h"

namespace {

using htf_nlist::kEmpty;

constexpr float kMaxImages = 64.f; // |x_c| <= 64 L_c: binned by position; anything else is in the extra cell
constexpr unsigned kRanges = 28;   // 27 stencil cells + the extra cell

// the word offsets of the scratch's parts (cell_of, order, cell_start, the sort's scratch, the cell-ordered copy)
struct Layout {
    size_t cell_of, order, cell_start, sort, sorted, total;
};

__host__ __device__ inline size_t round4(size_t w) { return (w + 3u) & ~(size_t)3u; }

inline Layout layout(unsigned M, unsigned ncell) {
    Layout l;
    l.cell_of = 0;
    l.order = round4(M);
    l.cell_start = l.order + round4(M);
    l.sort = l.cell_start + round4((size_t)ncell + 2u);
    l.sorted = l.sort + round4(2u * ((size_t)ncell + 1u));
    l.total = l.sorted + 4u * (size_t)M;
    return l;
}

// cell_of[i]: x fastest; the extra cell nx * ny * nz for a row outside [-64 L, 64 L] or not finite
__global__ __launch_bounds__(256) void nlist_bin_kernel(const float *__restrict__ pos, unsigned stride, unsigned M,
                                                        const float *__restrict__ box_L, unsigned nx, unsigned ny, unsigned nz,
                                                        unsigned *__restrict__ cell_of) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const unsigned n[3] = {nx, ny, nz};
    unsigned c[3];
    bool binned = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float x = pos[(size_t)i * stride + d], L = box_L[d];
        binned = binned && fabsf(x) <= kMaxImages * L; // (false for NaN and inf)
        const double t = binned ? (double)x / (double)L : 0.0;
        const double f = t - floor(t); // in [0, 1]
        c[d] = min((unsigned)(f * (double)n[d]), n[d] - 1u);
    }
    cell_of[i] = binned ? c[0] + nx * (c[1] + ny * c[2]) : nx * ny * nz;
}

// the cell-ordered candidates: (x, y, z, index bits)
__global__ __launch_bounds__(256) void nlist_gather_kernel(const float *__restrict__ pos, unsigned stride, unsigned M,
                                                           const unsigned *__restrict__ order, float4 *__restrict__ sorted) {
    const unsigned s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= M) return;
    const unsigned j = order[s];
    sorted[s] = make_float4(pos[(size_t)j * stride + 0], pos[(size_t)j * stride + 1], pos[(size_t)j * stride + 2], __uint_as_float(j));
}

// One wave per row, rows taken in cell order (slot s of the sort), so that the four waves of a workgroup -- and the
// workgroups beside it -- read the same few cells.  Lanes 0..27 each own one candidate range (a stencil cell, or the extra
// cell); their counts are scanned across the wave and every 64 consecutive candidates of the concatenated ranges are one
// step: lane q finds its range by a binary search of the prefix in LDS, measures the pair and the wave offers the keys.
template <int K>
__global__ __launch_bounds__(256) void nlist_cells_kernel(const float *__restrict__ pos, unsigned stride, unsigned M,
                                                          const float *__restrict__ box_L, float r_cut, unsigned nx, unsigned ny,
                                                          unsigned nz, unsigned NN, int sorted, int return_types,
                                                          const unsigned char *__restrict__ excl, const unsigned *__restrict__ cell_of,
                                                          const unsigned *__restrict__ cell_start, const unsigned *__restrict__ order,
                                                          const float4 *__restrict__ cand_pos, float *__restrict__ out,
                                                          int *__restrict__ out_idx) {
    __shared__ unsigned s_beg[4][32], s_pre[4][32];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned slot = blockIdx.x * 4u + wave;
    const bool row_ok = slot < M; // wave-uniform
    const unsigned ncell = nx * ny * nz;
    const float Lx = box_L[0], Ly = box_L[1], Lz = box_L[2];
    unsigned i = 0, beg = 0, cnt = 0;
    float xi = 0.f, yi = 0.f, zi = 0.f;
    if (row_ok) {
        i = order[slot];
        xi = pos[(size_t)i * stride + 0];
        yi = pos[(size_t)i * stride + 1];
        zi = pos[(size_t)i * stride + 2];
        const unsigned c = cell_of[i];
        if (c == ncell) { // a row in the extra cell: every candidate
            if (lane == 0) cnt = M;
        } else if (lane < 27u) {
            const unsigned cx = c % nx, cy = (c / nx) % ny, cz = c / (nx * ny);
            const unsigned ax = (cx + nx + lane % 3u - 1u) % nx, ay = (cy + ny + (lane / 3u) % 3u - 1u) % ny,
                           az = (cz + nz + lane / 9u - 1u) % nz;
            const unsigned cc = ax + nx * (ay + ny * az);
            beg = cell_start[cc];
            cnt = cell_start[cc + 1u] - beg;
        } else if (lane == 27u) {
            beg = cell_start[ncell];
            cnt = cell_start[ncell + 1u] - beg;
        }
    }
    unsigned incl = cnt; // inclusive scan over the lanes (only lanes < kRanges hold a range)
#pragma unroll
    for (unsigned off = 1; off < 32u; off <<= 1) {
        const unsigned v = (unsigned)__shfl_up((int)incl, off);
        if (lane >= off) incl += v;
    }
    const unsigned total = (unsigned)__shfl((int)incl, 31);
    if (lane < 32u) {
        s_beg[wave][lane] = beg;
        s_pre[wave][lane] = incl - cnt; // exclusive
    }
    __syncthreads();

    unsigned long long key[K];
#pragma unroll
    for (int k = 0; k < K; ++k) key[k] = kEmpty;
    unsigned long long worst = kEmpty;
    const unsigned last_k = (NN - 1u) >> 6, last_lane = (NN - 1u) & 63u;
    const unsigned *pre = s_pre[wave];
    for (unsigned base = 0; base < total; base += 64u) {
        const unsigned q = base + lane;
        unsigned long long cand = kEmpty;
        if (q < total) {
            unsigned r = 0; // the last range starting at or before q (prefix non-decreasing: a non-empty one)
#pragma unroll
            for (unsigned step = 16; step; step >>= 1)
                if (r + step < kRanges && pre[r + step] <= q) r += step;
            const float4 cj = cand_pos[s_beg[wave][r] + (q - pre[r])];
            const unsigned j = __float_as_uint(cj.w);
            cand = htf_nlist::key_of(htf_nlist::pair_of(xi, yi, zi, cj.x, cj.y, cj.z, Lx, Ly, Lz), r_cut, sorted, excl, i, j, M);
        }
        htf_nlist::offer<K>(key, worst, cand, lane, NN, last_k, last_lane);
    }
    if (!row_ok) return;
    htf_nlist::write_row<K>(key, lane, i, NN, pos, stride, xi, yi, zi, Lx, Ly, Lz, return_types, out, out_idx);
}

} // namespace

extern "C" unsigned long long htf_nlist_cells_scratch_words(unsigned M, unsigned ncell) { return layout(M, ncell).total; }

extern "C" int htf_nlist_cells_forward(const float *d_pos, unsigned pos_stride, unsigned M, const float *d_box_L, float r_cut,
                                       unsigned nx, unsigned ny, unsigned nz, unsigned NN, int sorted, int return_types,
                                       const unsigned char *d_excl, unsigned *d_scratch, float *d_out, int *d_idx,
                                       htf_stream stream) {
    HTF_REQUIRE(d_pos && d_box_L && d_scratch && d_out && d_idx, "htf_nlist_cells_forward: null pointer");
    HTF_REQUIRE(M >= 1, "htf_nlist_cells_forward: M must be >= 1");
    HTF_REQUIRE(NN >= 1 && NN <= 256, "htf_nlist_cells_forward: NN must be in [1, 256] (got %u)", NN);
    HTF_REQUIRE(pos_stride >= (return_types ? 4u : 3u), "htf_nlist_cells_forward: pos_stride %u too small", pos_stride);
    HTF_REQUIRE(nx >= 3 && ny >= 3 && nz >= 3, "htf_nlist_cells_forward: every dimension needs >= 3 cells (got %u x %u x %u)",
                nx, ny, nz);
    HTF_REQUIRE((unsigned long long)nx * ny * nz < 0xFFFFFFFEull, "htf_nlist_cells_forward: too many cells");
    HTF_REQUIRE(((uintptr_t)d_scratch & 15) == 0, "htf_nlist_cells_forward: scratch must be 16-byte aligned");
    const unsigned ncell = nx * ny * nz;
    const Layout l = layout(M, ncell);
    unsigned *cell_of = d_scratch + l.cell_of, *order = d_scratch + l.order, *cell_start = d_scratch + l.cell_start;
    float4 *cand = reinterpret_cast<float4 *>(d_scratch + l.sorted);
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(nlist_bin_kernel, dim3((M + 255) / 256), dim3(256), 0, s, d_pos, pos_stride, M, d_box_L, nx, ny, nz, cell_of);
    if (int rc = htf::check_launch("nlist_bin_kernel")) return rc;
    // cells 0 .. ncell - 1 and the extra cell ncell: ascending index inside a cell (deterministic)
    if (int rc = htfs_cell_sort(cell_of, M, ncell + 1u, d_scratch + l.sort, cell_start, order, stream)) return rc;
    hipLaunchKernelGGL(nlist_gather_kernel, dim3((M + 255) / 256), dim3(256), 0, s, d_pos, pos_stride, M, order, cand);
    if (int rc = htf::check_launch("nlist_gather_kernel")) return rc;
    const dim3 grid((M + 3) / 4), block(256);
    switch ((NN + 63) / 64) {
    case 1: hipLaunchKernelGGL(nlist_cells_kernel<1>, grid, block, 0, s, d_pos, pos_stride, M, d_box_L, r_cut, nx, ny, nz, NN, sorted, return_types, d_excl, cell_of, cell_start, order, cand, d_out, d_idx); break;
    case 2: hipLaunchKernelGGL(nlist_cells_kernel<2>, grid, block, 0, s, d_pos, pos_stride, M, d_box_L, r_cut, nx, ny, nz, NN, sorted, return_types, d_excl, cell_of, cell_start, order, cand, d_out, d_idx); break;
    case 3: hipLaunchKernelGGL(nlist_cells_kernel<3>, grid, block, 0, s, d_pos, pos_stride, M, d_box_L, r_cut, nx, ny, nz, NN, sorted, return_types, d_excl, cell_of, cell_start, order, cand, d_out, d_idx); break;
    default: hipLaunchKernelGGL(nlist_cells_kernel<4>, grid, block, 0, s, d_pos, pos_stride, M, d_box_L, r_cut, nx, ny, nz, NN, sorted, return_types, d_excl, cell_of, cell_start, order, cand, d_out, d_idx); break;
    }
    return htf::check_launch("nlist_cells_kernel");
}
