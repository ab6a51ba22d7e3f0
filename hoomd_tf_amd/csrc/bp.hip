// The descriptor network (include/htf_bp.h, htf.DescriptorMLP): per particle, D = n_types * K Gaussian channel sums of the
// neighbor distances -> Dense(H1) -> Dense(H2) -> Dense(1) = E_i, forces F_i = 2 sum_j dE_i/dx_ij (compute_nlist_forces), and
// the force-matching sweep over the same rows.  The layer's one translation unit.
//
// The rows themselves are desc_row.h's (forces, descriptor) and dtrain_row.h's (sweep), instantiated here with the cutoff on
// or off and with or without a row list (selected by d_rows alone).  One network per species is one launch per species:
// Python partitions the batch into ascending row lists and passes each with its species' weights.  Every output row is
// written by the one launch that lists it: no memset, no atomics.  The sweep's partials are a function of n_rows alone and
// the reduction below adds them in a fixed order, so entry q of the list is row q of a batch of n_rows, bit for bit.
// Built with -ffp-contract=on (csrc/Makefile).
#include "htf_bp.h"
#include "desc_row.h"
#include "dtrain_row.h"

namespace htf {
namespace {

template <bool FORCES, bool TANH, bool VIRIAL, bool CUT, bool LIST, typename IT>
__global__ __launch_bounds__(256) void bp_rows_kernel(const typename Vec4<IT>::type *__restrict__ nlist, const int *__restrict__ rows,
                                                      unsigned n, unsigned NN, const float *__restrict__ weights,
                                                      const float *__restrict__ mu, int K, int T, int H1, int H2, float gap, float rc,
                                                      void *__restrict__ out, int out_f64, void *__restrict__ virial9) {
    desc_rows<FORCES, TANH, VIRIAL, CUT, LIST, IT>(nlist, rows, n, NN, weights, mu, K, T, H1, H2, gap, rc, out, out_f64, virial9);
}

template <bool TANH, bool CUT, bool LIST, typename IT>
__global__ __launch_bounds__(256, 1) void bp_sweep_kernel(const typename Vec4<IT>::type *__restrict__ nlist, const int *__restrict__ rows,
                                                          unsigned n, unsigned NN, const float *__restrict__ weights,
                                                          const float *__restrict__ mu, int K, int T, int H1, int H2, float gap, float rc,
                                                          const void *__restrict__ labels, int labels_f64,
                                                          const float4 *__restrict__ pred, float *__restrict__ partials) {
    dtrain_rows<TANH, CUT, LIST, IT>(nlist, rows, n, NN, weights, mu, K, T, H1, H2, gap, rc, labels, labels_f64, pred, partials);
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

// nparts may be 0: accum is then zero-filled (declared in htf_internal.h: ctrain.hip's sweep ends in the same reduction)
int dtrain_reduce_launch(const float *d_partials, unsigned nparts, unsigned n, float *d_accum, hipStream_t stream) {
    hipLaunchKernelGGL(dtrain_reduce_kernel, dim3((n + 63u) / 64u), dim3(256), 0, stream, d_partials, nparts, n, d_accum);
    return check_launch("dtrain_reduce_kernel");
}

} // namespace htf

extern "C" int htf_bp_forces(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types, unsigned H1,
                             unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap, void *d_force,
                             int force_dtype, void *d_virial9, const int *d_rows, unsigned n_rows, float r_cut, htf_stream stream) {
    using namespace htf;
    int rc = desc_check(d_nlist, nlist_dtype, B, NN, K, n_types, d_mu, gap, d_force, force_dtype);
    if (rc != HTF_OK) return rc;
    if ((rc = desc_check_network(d_weights, H1, H2, activation)) != HTF_OK) return rc;
    if ((rc = desc_check_rows(B, n_rows, r_cut)) != HTF_OK) return rc;
    if (n_rows == 0) return HTF_OK;
    const size_t lds = desc_lds_forces(K, n_types, H1, H2);
    const int out_f64 = force_dtype == HTF_F64;
    const hipStream_t s = (hipStream_t)stream;
    dispatch_flags([&](auto TANH, auto VIR, auto CUT, auto LIST, auto F64) {
        using IT = scalar_t<F64>;
        hipLaunchKernelGGL((bp_rows_kernel<true, TANH, VIR, CUT, LIST, IT>), dim3(desc_grid(n_rows)), dim3(256), lds, s,
                           (const typename Vec4<IT>::type *)d_nlist, d_rows, n_rows, NN, d_weights, d_mu, (int)K, (int)n_types, (int)H1,
                           (int)H2, gap, r_cut, d_force, out_f64, d_virial9);
    }, activation == HTF_ACT_TANH, d_virial9 != nullptr, r_cut > 0.0f, d_rows != nullptr, nlist_dtype == HTF_F64);
    return check_launch("bp_rows_kernel");
}

extern "C" int htf_bp_descriptor(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types,
                                 const float *d_mu, float gap, void *d_out, int out_dtype, float r_cut, htf_stream stream) {
    using namespace htf;
    int rc = desc_check(d_nlist, nlist_dtype, B, NN, K, n_types, d_mu, gap, d_out, out_dtype);
    if (rc != HTF_OK) return rc;
    if ((rc = desc_check_rows(B, B, r_cut)) != HTF_OK) return rc;
    if (B == 0) return HTF_OK;
    const size_t lds = desc_lds_descriptor(K);
    const int out_f64 = out_dtype == HTF_F64;
    const hipStream_t s = (hipStream_t)stream;
    dispatch_flags([&](auto CUT, auto F64) {
        using IT = scalar_t<F64>;
        hipLaunchKernelGGL((bp_rows_kernel<false, false, false, CUT, false, IT>), dim3(desc_grid(B)), dim3(256), lds, s,
                           (const typename Vec4<IT>::type *)d_nlist, (const int *)nullptr, B, NN, (const float *)nullptr, d_mu, (int)K,
                           (int)n_types, 0, 0, gap, r_cut, d_out, out_f64, nullptr);
    }, r_cut > 0.0f, nlist_dtype == HTF_F64);
    return check_launch("bp_rows_kernel");
}

extern "C" size_t htf_bp_scratch_floats(unsigned n_rows, unsigned K, unsigned n_types, unsigned H1, unsigned H2) {
    using namespace htf;
    if (dtrain_check(K, n_types, H1, H2) != HTF_OK) return 0;
    return (size_t)dtrain_grid(n_rows) * (1 + (size_t)dtrain_params(K * n_types, H1, H2));
}

extern "C" int htf_bp_loss_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types, unsigned H1,
                                unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap, const void *d_labels,
                                int labels_dtype, const float *d_pred, float *d_accum, float *d_scratch, const int *d_rows,
                                unsigned n_rows, float r_cut, htf_stream stream) {
    using namespace htf;
    int rc = dtrain_check_call(d_nlist, nlist_dtype, B, NN, K, n_types, H1, H2, activation, d_weights, d_mu, gap, d_labels, labels_dtype,
                               d_pred, d_accum, d_scratch);
    if (rc != HTF_OK) return rc;
    if ((rc = desc_check_rows(B, n_rows, r_cut)) != HTF_OK) return rc;
    if (!d_accum) return HTF_OK;   // (B = 0 and nothing to zero-fill: no launch)
    const unsigned n = 1u + dtrain_params(K * n_types, H1, H2);
    const unsigned grid = dtrain_grid(n_rows);   // (0 for no rows: the reduction alone then writes zeros)
    const hipStream_t s = (hipStream_t)stream;
    if (grid) {
        const size_t lds = dtrain_lds(K, n_types, H1, H2);
        const int l64 = labels_dtype == HTF_F64;
        dispatch_flags([&](auto TANH, auto CUT, auto LIST, auto F64) {
            using IT = scalar_t<F64>;
            hipLaunchKernelGGL((bp_sweep_kernel<TANH, CUT, LIST, IT>), dim3(grid), dim3(256), lds, s,
                               (const typename Vec4<IT>::type *)d_nlist, d_rows, n_rows, NN, d_weights, d_mu, (int)K, (int)n_types,
                               (int)H1, (int)H2, gap, r_cut, d_labels, l64, (const float4 *)d_pred, d_scratch);
        }, activation == HTF_ACT_TANH, r_cut > 0.0f, d_rows != nullptr, nlist_dtype == HTF_F64);
        const int rl = check_launch("bp_sweep_kernel");
        if (rl != HTF_OK) return rl;
    }
    return dtrain_reduce_launch(d_scratch, grid, n, d_accum, s);
}
