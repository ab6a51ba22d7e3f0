// The descriptor network (include/htf_desc.h, htf.DescriptorMLP): per particle, D = n_types * K Gaussian channel sums of the
// neighbor distances -> Dense(H1) -> Dense(H2) -> Dense(1) = E_i, forces F_i = 2 sum_j dE_i/dx_ij (compute_nlist_forces).
//
// The rows themselves -- layout, stages, what is recomputed and why -- are desc_row.h's, shared with bp.hip (the same network
// with a cutoff and over a row list, include/htf_bp.h).  This file instantiates them with both of those switches off.
#include "htf_desc.h"
#include "desc_row.h"

namespace htf {
namespace {

// FORCES = false: G alone, written to out [B][D].  FORCES = true: out [B][4] (f, E) and, with VIRIAL, virial9 [B][9].
template <bool FORCES, bool TANH, bool VIRIAL, typename IT>
__global__ __launch_bounds__(256) void desc_mlp_kernel(const typename Vec4<IT>::type *__restrict__ nlist, unsigned B, unsigned NN,
                                                       const float *__restrict__ weights, const float *__restrict__ mu, int K,
                                                       int T, int H1, int H2, float gap, void *__restrict__ out, int out_f64,
                                                       void *__restrict__ virial9) {
    desc_rows<FORCES, TANH, VIRIAL, false, false, IT>(nlist, nullptr, B, NN, weights, mu, K, T, H1, H2, gap, 0.f, out, out_f64, virial9);
}

} // namespace
} // namespace htf

extern "C" int htf_desc_forces(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types,
                               unsigned H1, unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap,
                               void *d_force, int force_dtype, void *d_virial9, htf_stream stream) {
    using namespace htf;
    const int rc = desc_check(d_nlist, nlist_dtype, B, NN, K, n_types, d_mu, gap, d_force, force_dtype);
    if (rc != HTF_OK) return rc;
    const int rn = desc_check_network(d_weights, H1, H2, activation);
    if (rn != HTF_OK) return rn;
    if (B == 0) return HTF_OK;
    const size_t lds = desc_lds_forces(K, n_types, H1, H2);
    const int out_f64 = force_dtype == HTF_F64;
    const hipStream_t s = (hipStream_t)stream;
#define HTF_DK(TANH, VIR, T, V4)                                                                                        \
    hipLaunchKernelGGL((desc_mlp_kernel<true, TANH, VIR, T>), dim3(desc_grid(B)), dim3(256), lds, s, (const V4 *)d_nlist, B, NN, \
                       d_weights, d_mu, (int)K, (int)n_types, (int)H1, (int)H2, gap, d_force, out_f64, d_virial9)
#define HTF_DK2(TANH, VIR)                                                                                              \
    do {                                                                                                                \
        if (nlist_dtype == HTF_F32) HTF_DK(TANH, VIR, float, float4); else HTF_DK(TANH, VIR, double, double4);          \
    } while (0)
    if (activation == HTF_ACT_TANH) {
        if (d_virial9) HTF_DK2(true, true); else HTF_DK2(true, false);
    } else {
        if (d_virial9) HTF_DK2(false, true); else HTF_DK2(false, false);
    }
#undef HTF_DK2
#undef HTF_DK
    return check_launch("desc_mlp_kernel");
}

extern "C" int htf_desc_descriptor(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types,
                                   const float *d_mu, float gap, void *d_out, int out_dtype, htf_stream stream) {
    using namespace htf;
    const int rc = desc_check(d_nlist, nlist_dtype, B, NN, K, n_types, d_mu, gap, d_out, out_dtype);
    if (rc != HTF_OK) return rc;
    if (B == 0) return HTF_OK;
    const size_t lds = desc_lds_descriptor(K);
    const int out_f64 = out_dtype == HTF_F64;
    const hipStream_t s = (hipStream_t)stream;
    if (nlist_dtype == HTF_F32)
        hipLaunchKernelGGL((desc_mlp_kernel<false, false, false, float>), dim3(desc_grid(B)), dim3(256), lds, s, (const float4 *)d_nlist,
                           B, NN, (const float *)nullptr, d_mu, (int)K, (int)n_types, 0, 0, gap, d_out, out_f64, nullptr);
    else
        hipLaunchKernelGGL((desc_mlp_kernel<false, false, false, double>), dim3(desc_grid(B)), dim3(256), lds, s, (const double4 *)d_nlist,
                           B, NN, (const float *)nullptr, d_mu, (int)K, (int)n_types, 0, 0, gap, d_out, out_f64, nullptr);
    return check_launch("desc_mlp_kernel");
}
