// Force matching for the descriptor network (include/htf_desc_train.h, htf.DescriptorMLP.loss_gradient): the sum of squared
// residuals of (F_i, E_i) against the labels and its gradient with respect to the weights, in one pass over the pair vectors.
//
// The rows themselves -- the value-and-tangent forward pass, the reverse pass, the register accumulators and the block's
// partial -- are dtrain_row.h's, shared with bp.hip (the same sweep with a cutoff and over a row list, include/htf_bp.h).
// This file instantiates them with both of those switches off and owns the reduction of the partials, which bp.hip launches too.
// Built with -ffp-contract=on like desc_mlp.o (csrc/Makefile).
#include "htf_desc_train.h"
#include "dtrain_row.h"

namespace htf {
namespace {

template <bool TANH, typename IT>
__global__ __launch_bounds__(256, 1) void dtrain_sweep_kernel(const typename Vec4<IT>::type *__restrict__ nlist, unsigned B, unsigned NN,
                                                              const float *__restrict__ weights, const float *__restrict__ mu, int K,
                                                              int T, int H1, int H2, float gap, const void *__restrict__ labels,
                                                              int labels_f64, const float4 *__restrict__ pred,
                                                              float *__restrict__ partials) {
    dtrain_rows<TANH, false, false, IT>(nlist, nullptr, B, NN, weights, mu, K, T, H1, H2, gap, 0.f, labels, labels_f64, pred, partials);
}

// accum[p] = sum over the blocks' partials, in a fixed order: wave w of a block adds partials w, w + 4, ... for 64 entries,
// then the four sums are added as (0 + 1) + (2 + 3).  The gradient entries carry the factor 2 of d SSR = 2 sum dQ.
__global__ __launch_bounds__(256) void dtrain_reduce_kernel(const float *__restrict__ partials, unsigned nparts, unsigned n,
                                                            float *__restrict__ accum) {
    __shared__ float s[4][64];
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const unsigned p = blockIdx.x * 64u + lane;
    float v = 0.f;
    if (p < n)
        for (unsigned g = wave; g < nparts; g += 4) v += partials[(size_t)g * n + p];
    s[wave][lane] = v;
    __syncthreads();
    if (wave == 0 && p < n) {
        const float t = (s[0][lane] + s[1][lane]) + (s[2][lane] + s[3][lane]);
        accum[p] = p == 0 ? t : 2.0f * t;
    }
}

} // namespace

int dtrain_reduce_launch(const float *d_partials, unsigned nparts, unsigned n, float *d_accum, hipStream_t stream) {
    hipLaunchKernelGGL(dtrain_reduce_kernel, dim3((n + 63u) / 64u), dim3(256), 0, stream, d_partials, nparts, n, d_accum);
    return check_launch("dtrain_reduce_kernel");
}

} // namespace htf

extern "C" size_t htf_dtrain_scratch_floats(unsigned B, unsigned K, unsigned n_types, unsigned H1, unsigned H2) {
    using namespace htf;
    if (dtrain_check(K, n_types, H1, H2) != HTF_OK) return 0;
    return (size_t)dtrain_grid(B) * (1 + (size_t)dtrain_params(K * n_types, H1, H2));
}

extern "C" int htf_dtrain_loss_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types,
                                    unsigned H1, unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap,
                                    const void *d_labels, int labels_dtype, const float *d_pred, float *d_accum, float *d_scratch,
                                    htf_stream stream) {
    using namespace htf;
    const int rc = dtrain_check_call(d_nlist, nlist_dtype, B, NN, K, n_types, H1, H2, activation, d_weights, d_mu, gap, d_labels,
                                     labels_dtype, d_pred, d_accum, d_scratch);
    if (rc != HTF_OK) return rc;
    if (B == 0 && !d_accum) return HTF_OK;   // (no rows and nothing to zero-fill: no launch)
    const int D = (int)(K * n_types);
    const unsigned n = 1u + dtrain_params((unsigned)D, H1, H2);
    const unsigned grid = dtrain_grid(B);   // (0 for B = 0: the second kernel alone then writes zeros)
    const hipStream_t s = (hipStream_t)stream;
    if (grid) {
        const size_t lds = dtrain_lds(K, n_types, H1, H2);
        const int l64 = labels_dtype == HTF_F64;
#define HTF_DT(TANH, T, V4)                                                                                                        \
    hipLaunchKernelGGL((dtrain_sweep_kernel<TANH, T>), dim3(grid), dim3(256), lds, s, (const V4 *)d_nlist, B, NN, d_weights, d_mu, \
                       (int)K, (int)n_types, (int)H1, (int)H2, gap, d_labels, l64, (const float4 *)d_pred, d_scratch)
        if (activation == HTF_ACT_TANH) {
            if (nlist_dtype == HTF_F32) HTF_DT(true, float, float4); else HTF_DT(true, double, double4);
        } else {
            if (nlist_dtype == HTF_F32) HTF_DT(false, float, float4); else HTF_DT(false, double, double4);
        }
#undef HTF_DT
        const int rl = check_launch("dtrain_sweep_kernel");
        if (rl != HTF_OK) return rl;
    }
    return dtrain_reduce_launch(d_scratch, grid, n, d_accum, s);
}
