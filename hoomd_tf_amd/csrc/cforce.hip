// Conservative forces of the descriptor network (include/htf_cforce.h, htf.DescriptorMLP(conservative=True)):
// F_i = -d(sum_j E_j)/dr_i in two sweeps over the pair vectors.
//
// Pass 1 is desc_row.h's row through step 4 (its GRAD switch): the network forward and backward of every listed row, one
// wave per row, g_i = dE_i/dG_i written from lanes < D and E_i from lane 0.  One launch per species, as htf_bp_forces.
//
// Pass 2 is one launch over all rows, one wave per row, slots in registers read by the row kernel's own desc_slot
// (the same r, fc, fc').  The wave stages its own g_i in its LDS line; each lane gathers, per slot, the
// K floats g[j][t_i K ..] of the slot's particle j -- one 4 K-byte run per lane from a table of B D floats, as float4 where K is
// a multiple of 4 (every run is then 16-byte aligned) -- and recomputes the exponentials as step 5 of the row kernel does.
// phi, F_i and W_i follow by the fixed-order wave sums and the store of desc_pair_force_end (desc_row.h), which
// angular.hip's pass 2 ends in too.  No atomics, no scratch: a row's bits depend on its slots, its
// indices and the gathered rows of g alone.  Built with -ffp-contract=on like bp.o (csrc/Makefile), so that pass 1 forms
// the energy bit for bit as the force kernel does.
#include "htf_cforce.h"
#include "htf_cghost.h"
#include "desc_row.h"

namespace htf {
namespace {

template <bool TANH, bool CUT, bool LIST, typename IT>
__global__ __launch_bounds__(256) void cf_grad_kernel(const typename Vec4<IT>::type *__restrict__ nlist, const int *__restrict__ rows,
                                                      unsigned n, unsigned NN, const float *__restrict__ weights,
                                                      const float *__restrict__ mu, int K, int T, int H1, int H2, float gap, float rc,
                                                      float *__restrict__ g, float *__restrict__ energy) {
    desc_rows<true, TANH, false, CUT, LIST, IT, true>(nlist, rows, n, NN, weights, mu, K, T, H1, H2, gap, rc, g, 0, energy);
}

// WIDE: K % 4 == 0 and g is 16-byte aligned (the launcher checks both): a slot's run of g is read as K / 4 float4.
// n_table >= B: the rows of g (include/htf_cghost.h); rows [B, n_table) are ghosts' rows, read through a slot's index only.
template <bool VIRIAL, bool CUT, bool WIDE, typename IT>
__global__ __launch_bounds__(256) void cf_pair_force_kernel(const typename Vec4<IT>::type *__restrict__ nlist,
                                                            const int *__restrict__ index, const float *__restrict__ types, unsigned B,
                                                            unsigned n_table, unsigned NN, const float *__restrict__ mu, int K, int T,
                                                            float gap, float rc, const float *__restrict__ g, const float *__restrict__ energy,
                                                            void *__restrict__ out, int out_f64, void *__restrict__ virial9) {
    extern __shared__ float s_mem[];
    constexpr int KV = WIDE ? 4 : 1;
    const int D = K * T;
    float *s_mu = s_mem;
    float *s_x = s_mu + ((K + 3) & ~3) + (threadIdx.x >> 6) * 64; // this wave's line: its own g_i
    for (int i = threadIdx.x; i < K; i += blockDim.x) s_mu[i] = mu[i];
    __syncthreads();

    const float c_exp = -1.4426950408889634f / gap; // exp(-d^2 / gap) = exp2(c_exp d^2)
    const float c_der = -2.0f / gap;                // d e / d r = c_der (r - mu) e
    const float c_fc = CUT ? cutoff_slope(rc) : 0.f;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned ns = (NN + 63u) >> 6;            // slots per lane in use (wave-uniform)
    const unsigned stride = gridDim.x * (blockDim.x >> 6);
    // the index bound in a vector register: as one more scalar held across the row loop it spilled two SGPRs in three forms
    unsigned n_index = n_table;
    asm volatile("" : "+v"(n_index));

    for (unsigned row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); row < B; row += stride) { // wave-uniform
        const typename Vec4<IT>::type *rp = nlist + (size_t)row * NN;
        const int *ip = index + (size_t)row * NN;

        // 1. this lane's slots, read by desc_row.h's desc_slot (the same r, fc and fc'), with a keep rule of its own: a slot
        //    is kept (near) on its distance alone, and a neighbor type outside [0, T) only empties its forward term (ty = -1) --
        //    the neighbor's own energy still depends on this row's particle
        float x[kDescSlots], y[kDescSlots], z[kDescSlots], r[kDescSlots];
        float fc[kDescSlots], dfc[kDescSlots];   // (CUT only)
        int ty[kDescSlots];
        bool near[kDescSlots];
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) {
            const unsigned slot = t * 64 + lane;
            x[t] = y[t] = z[t] = 0.f;
            r[t] = 1.f;
            fc[t] = dfc[t] = 0.f;
            ty[t] = -1;
            near[t] = false;
            if ((unsigned)t < ns && slot < NN) {
                const DescSlot s = desc_slot<IT>(&rp[slot], T);
                x[t] = s.x; y[t] = s.y; z[t] = s.z;
                bool live = s.rr > kRinvDelta;
                if constexpr (CUT) live = live && s.rr < rc;
                if (live) {
                    near[t] = true;
                    r[t] = s.rr;
                    ty[t] = s.typ;
                    if constexpr (CUT) cutoff_terms(s.rr, rc, c_fc, fc[t], dfc[t]);
                }
            }
        }

        // 2. where each slot's reverse term lives: g[j][t_i K ..], or nowhere (index outside [0, n_table), own type out of range)
        int ti = 0;
        if (T > 1) {
            const float tw = rintf(types[row]);
            ti = (tw >= 0.f && tw < (float)T) ? (int)tw : -1; // (NaN: -1)
        }
        const float *gj[kDescSlots];
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) {
            gj[t] = nullptr;
            if ((unsigned)t < ns && near[t] && ti >= 0) {   // (a kept slot: t * 64 + lane < NN)
                const int j = ip[t * 64 + lane];
                if ((unsigned)j < n_index) gj[t] = g + ((size_t)j * D + ti * K);
            }
        }
        line_publish(s_x, lane, (int)lane < D ? g[(size_t)row * D + lane] : 0.f);

        // 3. dE_total/dr of every slot: sum_k (g_i + g_j) d_k e_k and (CUT only) sum_k (g_i + g_j) e_k, exponentials recomputed
        float acc[kDescSlots], acc0[kDescSlots];
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) acc[t] = acc0[t] = 0.f;
        for (int k0 = 0; k0 < K; k0 += KV) {
            float gr[kDescSlots][KV];
#pragma unroll
            for (int t = 0; t < kDescSlots; ++t) {
#pragma unroll
                for (int kk = 0; kk < KV; ++kk) gr[t][kk] = 0.f;
                if ((unsigned)t < ns && gj[t] != nullptr) {
                    if constexpr (WIDE) {
                        const float4 v = *reinterpret_cast<const float4 *>(gj[t] + k0);
                        gr[t][0] = v.x; gr[t][1] = v.y; gr[t][2] = v.z; gr[t][3] = v.w;
                    } else {
                        gr[t][0] = gj[t][k0];
                    }
                }
            }
#pragma unroll
            for (int kk = 0; kk < KV; ++kk) {
                const int k = k0 + kk;
                const float m = s_mu[k];
#pragma unroll
                for (int t = 0; t < kDescSlots; ++t) {
                    if ((unsigned)t < ns) {
                        const float d = r[t] - m;
                        const float ev = __builtin_amdgcn_exp2f(c_exp * (d * d));
                        const float gi = s_x[(ty[t] > 0 ? ty[t] : 0) * K + k];
                        const float gk = (ty[t] >= 0 ? gi : 0.f) + gr[t][kk];
                        acc[t] = fmaf(gk * d, ev, acc[t]);
                        if constexpr (CUT) acc0[t] = fmaf(gk, ev, acc0[t]);
                    }
                }
            }
        }

        // 4. phi, F and W
        float fx = 0.f, fy = 0.f, fz = 0.f;
        float w[9];
#pragma unroll
        for (int c9 = 0; c9 < 9; ++c9) w[c9] = 0.f;
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) {
            if ((unsigned)t < ns && near[t]) {
                float c;
                if constexpr (CUT)
                    c = (fc[t] * (c_der * acc[t]) + dfc[t] * acc0[t]) / r[t];
                else
                    c = (c_der * acc[t]) / r[t];
                const float ax = c * (x[t] + kNormDelta), ay = c * (y[t] + kNormDelta), az = c * (z[t] + kNormDelta);
                fx += ax; fy += ay; fz += az;
                if constexpr (VIRIAL) {
                    const float hx = -0.5f * x[t], hy = -0.5f * y[t], hz = -0.5f * z[t];
                    w[0] += hx * ax; w[1] += hx * ay; w[2] += hx * az;
                    w[3] += hy * ax; w[4] += hy * ay; w[5] += hy * az;
                    w[6] += hz * ax; w[7] += hz * ay; w[8] += hz * az;
                }
            }
        }
        desc_pair_force_end<VIRIAL>(lane, row, fx, fy, fz, w, energy, out, out_f64, virial9);
    }
}

} // namespace
} // namespace htf

extern "C" int htf_cf_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types, unsigned H1,
                           unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap, float *d_g,
                           float *d_energy, const int *d_rows, unsigned n_rows, float r_cut, htf_stream stream) {
    using namespace htf;
    int rc = desc_check(d_nlist, nlist_dtype, B, NN, K, n_types, d_mu, gap, d_g, HTF_F32);
    if (rc != HTF_OK) return rc;
    if ((rc = desc_check_network(d_weights, H1, H2, activation)) != HTF_OK) return rc;
    if ((rc = desc_check_rows(B, n_rows, r_cut)) != HTF_OK) return rc;
    HTF_REQUIRE(B == 0 || d_energy, "descriptor network: null pointer");
    if (n_rows == 0) return HTF_OK;
    const size_t lds = desc_lds_forces(K, n_types, H1, H2);
    const hipStream_t s = (hipStream_t)stream;
    dispatch_flags([&](auto TANH, auto CUT, auto LIST, auto F64) {
        using IT = scalar_t<F64>;
        hipLaunchKernelGGL((cf_grad_kernel<TANH, CUT, LIST, IT>), dim3(desc_grid(n_rows)), dim3(256), lds, s,
                           (const typename Vec4<IT>::type *)d_nlist, d_rows, n_rows, NN, d_weights, d_mu, (int)K, (int)n_types, (int)H1,
                           (int)H2, gap, r_cut, d_g, d_energy);
    }, activation == HTF_ACT_TANH, r_cut > 0.0f, d_rows != nullptr, nlist_dtype == HTF_F64);
    return check_launch("cf_grad_kernel");
}

extern "C" int htf_cf_forces_ghost(const void *d_nlist, int nlist_dtype, const int *d_index, const float *d_types, unsigned B,
                                   unsigned NN, unsigned K, unsigned n_types, const float *d_mu, float gap, const float *d_g,
                                   const float *d_energy, void *d_force, int force_dtype, void *d_virial9, float r_cut,
                                   unsigned n_table, htf_stream stream) {
    using namespace htf;
    HTF_REQUIRE(n_table >= B, "descriptor network: n_table %u < B %u", n_table, B);
    int rc = desc_check(d_nlist, nlist_dtype, B, NN, K, n_types, d_mu, gap, d_force, force_dtype);
    if (rc != HTF_OK) return rc;
    if ((rc = desc_check_rows(B, B, r_cut)) != HTF_OK) return rc;
    HTF_REQUIRE(B == 0 || (d_index && d_g && d_energy), "descriptor network: null pointer");
    HTF_REQUIRE(B == 0 || n_types == 1 || d_types, "descriptor network: n_types = %u needs the rows' own types", n_types);
    if (B == 0) return HTF_OK;
    const size_t lds = desc_lds_descriptor(K);
    const int out_f64 = force_dtype == HTF_F64;
    const bool wide = K % 4u == 0 && ((uintptr_t)d_g & 15u) == 0;
    const hipStream_t s = (hipStream_t)stream;
    dispatch_flags([&](auto VIR, auto CUT, auto WIDE, auto F64) {
        using IT = scalar_t<F64>;
        hipLaunchKernelGGL((cf_pair_force_kernel<VIR, CUT, WIDE, IT>), dim3(desc_grid(B)), dim3(256), lds, s,
                           (const typename Vec4<IT>::type *)d_nlist, d_index, d_types, B, n_table, NN, d_mu, (int)K, (int)n_types, gap,
                           r_cut, d_g, d_energy, d_force, out_f64, d_virial9);
    }, d_virial9 != nullptr, r_cut > 0.0f, wide, nlist_dtype == HTF_F64);
    return check_launch("cf_pair_force_kernel");
}

// (the table is the pair tensor's own rows)
extern "C" int htf_cf_forces(const void *d_nlist, int nlist_dtype, const int *d_index, const float *d_types, unsigned B, unsigned NN,
                             unsigned K, unsigned n_types, const float *d_mu, float gap, const float *d_g, const float *d_energy,
                             void *d_force, int force_dtype, void *d_virial9, float r_cut, htf_stream stream) {
    return htf_cf_forces_ghost(d_nlist, nlist_dtype, d_index, d_types, B, NN, K, n_types, d_mu, gap, d_g, d_energy, d_force,
                               force_dtype, d_virial9, r_cut, B, stream);
}
