// Force matching on the conservative forces of the descriptor network (include/htf_ctrain.h,
// htf.DescriptorMLP.total_loss_gradient): d SSR / d theta for F = -d(sum_i E_i)/dr in one sweep over the pair vectors.
//
// The row is dtrain_row.h's with its TOTAL switch: the residual comes from a table [B][4], and a live slot reads the particle
// it holds and gathers that particle's residual, a = ((rho_i - rho_j) . t) / r.  Forward with tangent, reverse, register
// accumulators and block partials are the row sweep's; the partials are added by bp.hip's dtrain_reduce_kernel, the library's
// one reduction.  Every term lands on the row that reads it: no atomics, no scatter.  Built with -ffp-contract=on like bp.o
// (csrc/Makefile), so that the shared steps form the same values.
#include "htf_ctrain.h"
#include "htf_cghost.h"
#include "dtrain_row.h"

namespace htf {
namespace {

template <bool TANH, bool CUT, bool LIST, typename IT>
__global__ __launch_bounds__(256, 1) void ct_sweep_kernel(const typename Vec4<IT>::type *__restrict__ nlist, const int *__restrict__ index,
                                                          const int *__restrict__ rows, unsigned n, unsigned B, unsigned NN,
                                                          const float *__restrict__ weights, const float *__restrict__ mu, int K, int T,
                                                          int H1, int H2, float gap, float rc, const float4 *__restrict__ rho,
                                                          float *__restrict__ partials) {
    dtrain_rows<TANH, CUT, LIST, IT, true>(nlist, rows, n, NN, weights, mu, K, T, H1, H2, gap, rc, nullptr, 0, rho, partials, index, B);
}

} // namespace
} // namespace htf

// (the sweep has kept the row count n and the index bound apart from the start: the bound is the residual table's n_table rows)
extern "C" int htf_ct_loss_grad_ghost(const void *d_nlist, int nlist_dtype, const int *d_index, unsigned B, unsigned NN, unsigned K,
                                      unsigned n_types, unsigned H1, unsigned H2, int activation, const float *d_weights,
                                      const float *d_mu, float gap, const float *d_rho, float *d_accum, float *d_scratch,
                                      const int *d_rows, unsigned n_rows, float r_cut, unsigned n_table, htf_stream stream) {
    using namespace htf;
    HTF_REQUIRE(n_table >= B, "descriptor network: n_table %u < B %u", n_table, B);
    // (the residual table stands where htf_bp_loss_grad has the labels and the prediction)
    int rc = dtrain_check_call(d_nlist, nlist_dtype, B, NN, K, n_types, H1, H2, activation, d_weights, d_mu, gap, d_rho, HTF_F32, d_rho,
                               d_accum, d_scratch);
    if (rc != HTF_OK) return rc;
    HTF_REQUIRE(B == 0 || d_index, "descriptor network: null pointer");
    if ((rc = desc_check_rows(B, n_rows, r_cut)) != HTF_OK) return rc;
    if (!d_accum) return HTF_OK;   // (B = 0 and nothing to zero-fill: no launch)
    const unsigned n = 1u + dtrain_params(K * n_types, H1, H2);
    const unsigned grid = dtrain_grid(n_rows);   // (0 for no rows: the reduction alone then writes zeros)
    const hipStream_t s = (hipStream_t)stream;
    if (grid) {
        const size_t lds = dtrain_lds(K, n_types, H1, H2);
        dispatch_flags([&](auto TANH, auto CUT, auto LIST, auto F64) {
            using IT = scalar_t<F64>;
            hipLaunchKernelGGL((ct_sweep_kernel<TANH, CUT, LIST, IT>), dim3(grid), dim3(256), lds, s,
                               (const typename Vec4<IT>::type *)d_nlist, d_index, d_rows, n_rows, n_table, NN, d_weights, d_mu, (int)K,
                               (int)n_types, (int)H1, (int)H2, gap, r_cut, (const float4 *)d_rho, d_scratch);
        }, activation == HTF_ACT_TANH, r_cut > 0.0f, d_rows != nullptr, nlist_dtype == HTF_F64);
        const int rl = check_launch("ct_sweep_kernel");
        if (rl != HTF_OK) return rl;
    }
    return dtrain_reduce_launch(d_scratch, grid, n, d_accum, s);
}

extern "C" int htf_ct_loss_grad(const void *d_nlist, int nlist_dtype, const int *d_index, unsigned B, unsigned NN, unsigned K,
                                unsigned n_types, unsigned H1, unsigned H2, int activation, const float *d_weights, const float *d_mu,
                                float gap, const float *d_rho, float *d_accum, float *d_scratch, const int *d_rows, unsigned n_rows,
                                float r_cut, htf_stream stream) {
    return htf_ct_loss_grad_ghost(d_nlist, nlist_dtype, d_index, B, NN, K, n_types, H1, H2, activation, d_weights, d_mu, gap, d_rho,
                                  d_accum, d_scratch, d_rows, n_rows, r_cut, B, stream);
}
