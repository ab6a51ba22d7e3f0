// Coarse-grained mapping ops (include/htf_cg.h): the periodic centre of mass of a sparse mapping and an all-pairs neighbor
// list of the beads, forward and backward.
//
// Built with -ffp-contract=off (Makefile): the neighbor list must pick the same neighbors as the numpy restatement of
// utils.compute_nlist (oracle.compute_nlist), so every distance is formed as it is there -- fp32 differences,
// d - rint(d / L) * L, (x^2 + y^2) + z^2, sqrt -- with no fused multiply-add and correctly rounded division and square root.
// (sqrtf and '/', correctly rounded under HIP's default -fhip-fp32-correctly-rounded-divide-sqrt; __fsqrt_rn is not: it
// is the native ~1-ulp square root, which orders two neighbors whose distances differ by one ulp the wrong way round.)
#include "htf_common.h"
#include "htf_cg.h"
#include "nlist_select.h"

namespace {

constexpr float kTwoPi = 6.28318530717958647692f;
constexpr float kPi = 3.14159265358979323846f;
using htf_nlist::kEmpty;

// ------------------------------------------------------------------------------------------------ centre of mass
// G lanes per bead walk its CSR row; the sums meet by butterfly shuffles inside the lane group.
constexpr int kComLanes = 4;

__global__ __launch_bounds__(256) void com_forward_kernel(const float *__restrict__ pos, unsigned stride, unsigned B,
                                                          const int *__restrict__ row_ptr, const int *__restrict__ cols,
                                                          const float *__restrict__ vals, const float *__restrict__ box_L,
                                                          float *__restrict__ com, float *__restrict__ xz) {
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned b = t / kComLanes, g = t % kComLanes;
    const float L[3] = {box_L[0], box_L[1], box_L[2]};
    float X[3] = {0.f, 0.f, 0.f}, Z[3] = {0.f, 0.f, 0.f};
    if (b < B) {
        const int end = row_ptr[b + 1];
        for (int k = row_ptr[b] + (int)g; k < end; k += kComLanes) {
            const size_t a = (size_t)cols[k];
            const float w = vals[k];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float s, co;
                sincosf(__fmul_rn(__fdiv_rn(pos[a * stride + c], L[c]), kTwoPi), &s, &co);
                X[c] = __fadd_rn(X[c], __fmul_rn(w, co));
                Z[c] = __fadd_rn(Z[c], __fmul_rn(w, s));
            }
        }
    }
    // (every lane of the wave takes part in the shuffles, beads past B with zeros)
#pragma unroll
    for (int m = 1; m < kComLanes; m <<= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            X[c] = __fadd_rn(X[c], __shfl_xor(X[c], m));
            Z[c] = __fadd_rn(Z[c], __shfl_xor(Z[c], m));
        }
    }
    if (b < B && g == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float r = __fmul_rn(__fdiv_rn(__fdiv_rn(atan2f(Z[c], X[c]), kPi), 2.0f), L[c]);
            if (r <= -0.5f * L[c]) r = __fadd_rn(r, L[c]); // atan2 = -pi: the same point as +pi, reported as L/2
            com[(size_t)b * 3 + c] = r;
            if (xz) {
                xz[(size_t)b * 6 + c] = X[c];
                xz[(size_t)b * 6 + 3 + c] = Z[c];
            }
        }
    }
}

// one lane per atom walks its CSC column: every gradient entry is written once, in a fixed order
__global__ __launch_bounds__(256) void com_backward_kernel(const float *__restrict__ pos, unsigned stride, unsigned N,
                                                           const int *__restrict__ col_ptr, const int *__restrict__ rows,
                                                           const float *__restrict__ vals, const float *__restrict__ box_L,
                                                           const float *__restrict__ xz, const float *__restrict__ gcom,
                                                           float *__restrict__ gpos) {
    const unsigned a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= N) return;
    float sn[3], cs[3], acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c)
        sincosf(__fmul_rn(__fdiv_rn(pos[(size_t)a * stride + c], box_L[c]), kTwoPi), &sn[c], &cs[c]);
    const int end = col_ptr[a + 1];
    for (int k = col_ptr[a]; k < end; ++k) {
        const size_t b = (size_t)rows[k];
        const float w = vals[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float X = xz[b * 6 + c], Z = xz[b * 6 + 3 + c];
            const float r2 = __fadd_rn(__fmul_rn(X, X), __fmul_rn(Z, Z));
            if (r2 > 0.f) {
                const float num = __fmul_rn(w, __fadd_rn(__fmul_rn(X, cs[c]), __fmul_rn(Z, sn[c])));
                acc[c] = __fadd_rn(acc[c], __fmul_rn(__fdiv_rn(num, r2), gcom[b * 3 + c]));
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) gpos[(size_t)a * 3 + c] = acc[c];
}

// ------------------------------------------------------------------------------------------------ neighbor list
// One wave per row i streams all M candidates through an LDS tile the workgroup's four waves share; the row's list and its
// insertion step are nlist_select.h's (shared with the cell-binned search of nlist_cells.hip).
constexpr unsigned kTile = 256;

using htf_nlist::Pair;
using htf_nlist::pair_of;

template <int K>
__global__ __launch_bounds__(256) void nlist_forward_kernel(const float *__restrict__ pos, unsigned stride, unsigned M,
                                                            const float *__restrict__ box_L, float r_cut, unsigned NN, int sorted,
                                                            int return_types, const unsigned char *__restrict__ excl,
                                                            float *__restrict__ out, int *__restrict__ out_idx) {
    __shared__ float tx[kTile], ty[kTile], tz[kTile];
    const unsigned lane = threadIdx.x & 63u;
    const unsigned i = blockIdx.x * (blockDim.x / 64u) + (threadIdx.x >> 6);
    const bool row_ok = i < M; // wave-uniform
    const float Lx = box_L[0], Ly = box_L[1], Lz = box_L[2];
    float xi = 0.f, yi = 0.f, zi = 0.f;
    if (row_ok) {
        xi = pos[(size_t)i * stride + 0];
        yi = pos[(size_t)i * stride + 1];
        zi = pos[(size_t)i * stride + 2];
    }
    unsigned long long key[K];
#pragma unroll
    for (int k = 0; k < K; ++k) key[k] = kEmpty;
    unsigned long long worst = kEmpty; // key of slot NN - 1 (kEmpty until the list is full)
    const unsigned last_k = (NN - 1u) >> 6, last_lane = (NN - 1u) & 63u;

    for (unsigned base = 0; base < M; base += kTile) {
        __syncthreads(); // (the previous tile has been read by every wave)
        {
            const unsigned j = base + threadIdx.x;
            if (threadIdx.x < kTile && j < M) {
                tx[threadIdx.x] = pos[(size_t)j * stride + 0];
                ty[threadIdx.x] = pos[(size_t)j * stride + 1];
                tz[threadIdx.x] = pos[(size_t)j * stride + 2];
            }
        }
        __syncthreads();
        if (!row_ok) continue;
        const unsigned n_tile = min(kTile, M - base);
        for (unsigned sub = 0; sub < n_tile; sub += 64u) {
            const unsigned t = sub + lane, j = base + t;
            unsigned long long cand = kEmpty;
            if (t < n_tile) cand = htf_nlist::key_of(pair_of(xi, yi, zi, tx[t], ty[t], tz[t], Lx, Ly, Lz), r_cut, sorted, excl, i, j, M);
            htf_nlist::offer<K>(key, worst, cand, lane, NN, last_k, last_lane);
        }
    }
    if (!row_ok) return;
    htf_nlist::write_row<K>(key, lane, i, NN, pos, stride, xi, yi, zi, Lx, Ly, Lz, return_types, out, out_idx);
}

__global__ __launch_bounds__(256) void nlist_backward_kernel(const int *__restrict__ idx, unsigned M, unsigned NN,
                                                             const float *__restrict__ gout, float *__restrict__ gpos) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)M * NN) return;
    const int j = idx[t];
    if (j < 0) return;
    const size_t i = t / NN;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float g = gout[t * 4 + c];
        if (g != 0.f) {
            unsafeAtomicAdd(&gpos[i * 3 + c], -g);
            unsafeAtomicAdd(&gpos[(size_t)j * 3 + c], g);
        }
    }
}

} // namespace

extern "C" int htf_cg_com_forward(const float *d_pos, unsigned pos_stride, unsigned N, unsigned B, const int *d_row_ptr,
                                  const int *d_cols, const float *d_vals, const float *d_box_L, float *d_com, float *d_xz,
                                  htf_stream stream) {
    HTF_REQUIRE(d_row_ptr && d_box_L && d_com, "htf_cg_com_forward: null pointer");
    HTF_REQUIRE(pos_stride >= 3, "htf_cg_com_forward: pos_stride must be >= 3 (got %u)", pos_stride);
    if (B == 0) return HTF_OK;
    HTF_REQUIRE(N > 0 && d_pos && d_cols && d_vals, "htf_cg_com_forward: a mapping with %u beads needs atoms", B);
    const size_t threads = (size_t)B * kComLanes;
    hipLaunchKernelGGL(com_forward_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_pos,
                       pos_stride, B, d_row_ptr, d_cols, d_vals, d_box_L, d_com, d_xz);
    return htf::check_launch("com_forward_kernel");
}

extern "C" int htf_cg_com_backward(const float *d_pos, unsigned pos_stride, unsigned N, unsigned B, const int *d_col_ptr,
                                   const int *d_rows, const float *d_vals, const float *d_box_L, const float *d_xz,
                                   const float *d_grad_com, float *d_grad_pos, htf_stream stream) {
    HTF_REQUIRE(d_pos && d_col_ptr && d_box_L && d_grad_pos, "htf_cg_com_backward: null pointer");
    HTF_REQUIRE(pos_stride >= 3, "htf_cg_com_backward: pos_stride must be >= 3 (got %u)", pos_stride);
    if (N == 0) return HTF_OK;
    HTF_REQUIRE(B == 0 || (d_rows && d_vals && d_xz && d_grad_com), "htf_cg_com_backward: null pointer");
    (void)B;
    hipLaunchKernelGGL(com_backward_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_pos, pos_stride, N,
                       d_col_ptr, d_rows, d_vals, d_box_L, d_xz, d_grad_com, d_grad_pos);
    return htf::check_launch("com_backward_kernel");
}

extern "C" int htf_cg_nlist_forward(const float *d_pos, unsigned pos_stride, unsigned M, const float *d_box_L, float r_cut,
                                    unsigned NN, int sorted, int return_types, const unsigned char *d_excl, float *d_out,
                                    int *d_idx, htf_stream stream) {
    HTF_REQUIRE(d_pos && d_box_L && d_out && d_idx, "htf_cg_nlist_forward: null pointer");
    HTF_REQUIRE(M >= 1, "htf_cg_nlist_forward: M must be >= 1");
    HTF_REQUIRE(NN >= 1 && NN <= HTF_CG_MAX_NN, "htf_cg_nlist_forward: NN must be in [1, %d] (got %u)", HTF_CG_MAX_NN, NN);
    HTF_REQUIRE(pos_stride >= (return_types ? 4u : 3u), "htf_cg_nlist_forward: pos_stride %u too small", pos_stride);
    const dim3 grid((M + 3) / 4), block(256);
    const hipStream_t s = (hipStream_t)stream;
    switch ((NN + 63) / 64) {
    case 1: hipLaunchKernelGGL(nlist_forward_kernel<1>, grid, block, 0, s, d_pos, pos_stride, M, d_box_L, r_cut, NN, sorted, return_types, d_excl, d_out, d_idx); break;
    case 2: hipLaunchKernelGGL(nlist_forward_kernel<2>, grid, block, 0, s, d_pos, pos_stride, M, d_box_L, r_cut, NN, sorted, return_types, d_excl, d_out, d_idx); break;
    case 3: hipLaunchKernelGGL(nlist_forward_kernel<3>, grid, block, 0, s, d_pos, pos_stride, M, d_box_L, r_cut, NN, sorted, return_types, d_excl, d_out, d_idx); break;
    default: hipLaunchKernelGGL(nlist_forward_kernel<4>, grid, block, 0, s, d_pos, pos_stride, M, d_box_L, r_cut, NN, sorted, return_types, d_excl, d_out, d_idx); break;
    }
    return htf::check_launch("nlist_forward_kernel");
}

extern "C" int htf_cg_nlist_backward(const int *d_idx, unsigned M, unsigned NN, const float *d_grad_out, float *d_grad_pos,
                                     htf_stream stream) {
    HTF_REQUIRE(d_idx && d_grad_out && d_grad_pos, "htf_cg_nlist_backward: null pointer");
    HTF_REQUIRE(NN >= 1 && NN <= HTF_CG_MAX_NN, "htf_cg_nlist_backward: NN must be in [1, %d] (got %u)", HTF_CG_MAX_NN, NN);
    const size_t n = (size_t)M * NN;
    if (n == 0) return HTF_OK;
    hipLaunchKernelGGL(nlist_backward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_idx, M, NN,
                       d_grad_out, d_grad_pos);
    return htf::check_launch("nlist_backward_kernel");
}
