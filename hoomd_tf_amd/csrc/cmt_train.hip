// Force matching for every member of a committee of descriptor networks in one sweep (include/htf_cmt_train.h,
// htf.DescriptorMLP.committee_loss_gradient): {SSR^m, d SSR^m / d theta^m} of ctrain.hip's sweep for M networks at once.
//
// A block is one wave per member, and the block's waves walk the same rows in the same order.  Steps 1, 3 and 4 of a row are
// dtrain_row.h's with its TOTAL switch, member by member: every wave reads the row's slots (from HBM once, from the caches for the
// other waves), forms its member's a = ((rho_i - rho_j) . t) / r from its own float4 of the 16 M-byte residual records, and runs
// its member's network -- staged in LDS once per block, desc_lds_weights' layout -- forward with tangent and in reverse, with
// its own exchange lines and its own 128 register accumulators (M sets do not fit one wave, which is why a member has a wave).
// Step 2, the descriptor and its tangent, is shared by the block: e_k(r) and R'_k(r) do not depend on the member, so the waves
// split the K centres (wave m takes k = m, m + M, ...), each forms the exponentials of its centres once, G[c] once and
// Gdot^mm[c] = sum_s R'_k(s) a^mm(s) for every member mm from the a's the waves published in LDS, and writes them straight into
// member mm's exchange lines: K ns exponentials and K T (M + 1) wave sums per row for the block, where M separate sweeps take
// M K ns and 2 M K T.  Two block barriers per row.  Each wave writes its member's block partial itself -- the cross-wave add of
// dtrain_rows' step 5 has nothing to add.  The partials of member m, [grid][1 + P] at d_scratch + m * grid * (1 + P), are added
// by a second instance of bp.hip's dtrain_reduce_kernel that takes the member from the grid: one launch for all M results.  No
// atomics, no memset.  Built with -ffp-contract=on like ctrain.o (csrc/Makefile).
#include "htf_cmt_train.h"
#include "dtrain_row.h"

namespace htf {
namespace {

constexpr int kCmtTrainMaxModels = HTF_CMT_MAX_MODELS;
constexpr int kCmtTrainSlots = 64 * kDescSlots;   // floats of one member's a of a row
constexpr unsigned kCmtTrainRowsPerBlock = 16;   // rows a block takes before the grid grows: dtrain_rows' 16 per wave
// the largest grid is what the chip holds at once, so that no block waits for a second round: 256 compute units of eight waves
// (two per SIMD at the sweep's 200-odd registers), a block of W waves being resident 8 / W times per unit -- 2048 waves where W
// divides eight, dtrain_rows' 512 blocks of four
constexpr unsigned kCmtTrainUnits = 256, kCmtTrainUnitWaves = 8;

// floats of one member's weights in LDS (desc_lds_weights, rounded up to a multiple of 4)
__host__ __device__ inline int cmt_train_lds_member(int D, int H1, int H2) { return (desc_lds_weights(D, H1, H2) + 3) & ~3; }

// n work items: rows 0 .. n - 1, or rows[0 .. n - 1] with LIST.  blockDim.x = 64 M: wave m is member m.
template <bool TANH, bool CUT, bool LIST, typename IT>
__global__ __launch_bounds__(64 * kCmtTrainMaxModels) void committee_train_kernel(
    const typename Vec4<IT>::type *__restrict__ nlist, const int *__restrict__ index, const int *__restrict__ rows, unsigned n, unsigned B,
    unsigned NN, const float *__restrict__ weights, unsigned w_stride, const float *__restrict__ mu, int K, int T, int H1, int H2,
    float gap, float rc, const float4 *__restrict__ rho, float *__restrict__ partials) {
    extern __shared__ float s_mem[];
    const int D = K * T;
    const int ld1 = H1 + 1, ld2 = H2 + 1;   // odd row strides, as dtrain_rows stages them
    const int nwm = cmt_train_lds_member(D, H1, H2);
    const unsigned M = blockDim.x >> 6, m = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    float *s_w = s_mem + (size_t)m * nwm;   // this wave's member
    float *s_mu = s_mem + (size_t)M * nwm;
    float *s_lines = s_mu + ((K + 3) & ~3);                   // every member's exchange lines: the centre step writes G and Gdot there
    float *s_x = s_lines + m * (kDtLines * 64);               // this wave's own
    float *s_a = s_lines + M * (kDtLines * 64);               // a^m of the row's slots, [M][kCmtTrainSlots]
    float *sG = s_x, *sGd = s_x + 64, *sH = s_x + 128, *sHd = s_x + 192, *sZ = s_x + 256, *sZd = s_x + 320;
    float *W1 = s_w, *b1 = W1 + D * ld1, *W2 = b1 + H1, *b2 = W2 + H1 * ld2, *W3 = b2 + H2;
    {   // (every wave stages its own member's network)
        const float *g_w = weights + (size_t)m * w_stride;
        const float *g_b1 = g_w + D * H1, *g_W2 = g_b1 + H1, *g_b2 = g_W2 + H1 * H2;
        for (int i = lane; i < D * H1; i += 64) W1[(i / H1) * ld1 + i % H1] = g_w[i];
        for (int i = lane; i < H1 * H2; i += 64) W2[(i / H2) * ld2 + i % H2] = g_W2[i];
        for (int i = lane; i < H1; i += 64) b1[i] = g_b1[i];
        for (int i = lane; i < 2 * H2 + 1; i += 64) b2[i] = g_b2[i]; // b2 | W3 | b3, contiguous in both
    }
    for (int i = threadIdx.x; i < K; i += blockDim.x) s_mu[i] = mu[i];
    sG[lane] = sGd[lane] = 0.f;   // (entries past D stay zero: the centre step writes entries [0, D) alone)
    __syncthreads();

    const float c_exp = -1.4426950408889634f / gap; // exp(-d^2 / gap) = exp2(c_exp d^2)
    const float c_der = -2.0f / gap;                // d e / d r = c_der (r - mu) e
    const float c_fc = CUT ? cutoff_slope(rc) : 0.f;
    const unsigned ns = (NN + 63u) >> 6;            // slots per lane in use (wave-uniform)

    // this member's share of the gradient: aW1[c] = dW1[c][lane], aW2[a] = dW2[a][lane]
    float aW1[64], aW2[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) aW1[i] = aW2[i] = 0.f;
    float ab1 = 0.f, ab2 = 0.f, aW3 = 0.f, ab3 = 0.f, assr = 0.f;

    for (unsigned q = blockIdx.x; q < n; q += gridDim.x) { // block-uniform: every wave of the block takes the same rows
        unsigned row = q;
        if constexpr (LIST) row = (unsigned)rows[q];
        // 0. this member's residual of the row (the same value in every lane)
        const float4 pr = rho[(size_t)row * M + m];
        const float rx = pr.x, ry = pr.y, rz = pr.z, re = pr.w;
        assr += (rx * rx + ry * ry) + (rz * rz + re * re);

        // 1. this lane's slots: distance, type (-1: contributes nothing), a = ((rho_i - rho_j) . t) / r
        const typename Vec4<IT>::type *rp = nlist + (size_t)row * NN;
        float r[kDescSlots], a[kDescSlots];
        float fc[kDescSlots], dfc[kDescSlots];   // (CUT only)
        int ty[kDescSlots];
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) {
            const unsigned slot = t * 64 + lane;
            r[t] = 1.f;
            a[t] = 0.f;
            fc[t] = dfc[t] = 0.f;
            ty[t] = -1;
            if ((unsigned)t < ns && slot < NN) {
                const DescSlot s = desc_slot<IT>(&rp[slot], T);
                bool live = s.rr > kRinvDelta && s.typ >= 0;
                if constexpr (CUT) live = live && s.rr < rc;
                if (live) {
                    r[t] = s.rr;
                    ty[t] = s.typ;
                    float ax = rx, ay = ry, az = rz;
                    const int j = index[(size_t)row * NN + slot];
                    if ((unsigned)j < B) {   // (a negative index is above B as unsigned)
                        const float4 rj = rho[(size_t)j * M + m];   // this member's float4 of particle j's record
                        ax -= rj.x; ay -= rj.y; az -= rj.z;
                    }
                    a[t] = (ax * s.tx + ay * s.tyy + az * s.tz) / s.rr;
                    if constexpr (CUT) cutoff_terms(s.rr, rc, c_fc, fc[t], dfc[t]);
                }
            }
        }

        // 2. G and Gdot, shared by the block: every wave publishes its member's a, then takes the centres k = m, m + M, ... and
        //    forms e_k and R'_k of its own slots once -- they do not depend on the member -- G[c] once, and Gdot^mm[c] =
        //    sum_s R'_k(s) a^mm(s) for every member mm, each straight into that member's exchange lines.  Two block barriers
        //    per row; the first also says that every wave has finished reading the previous row's lines.
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t)
            if ((unsigned)t < ns) s_a[m * kCmtTrainSlots + t * 64 + lane] = a[t];
        __syncthreads();
        for (int k = (int)m; k < K; k += (int)M) {   // wave-uniform
            const float cm = s_mu[k];
            float e[kDescSlots], er[kDescSlots];   // e_k and R'_k = (c_der d fc + fc') e_k of this lane's slots
#pragma unroll
            for (int t = 0; t < kDescSlots; ++t) {
                e[t] = er[t] = 0.f;
                if ((unsigned)t < ns) {
                    const float d = r[t] - cm;
                    const float ev = __builtin_amdgcn_exp2f(c_exp * (d * d));
                    const float el = ty[t] >= 0 ? ev : 0.f;
                    if constexpr (CUT) {
                        e[t] = fc[t] * el;
                        er[t] = ((c_der * d) * fc[t] + dfc[t]) * el;
                    } else {
                        e[t] = el;
                        er[t] = (c_der * d) * el;
                    }
                }
            }
            for (int tt = 0; tt < T; ++tt) {
                const int c = tt * K + k;
                float p = 0.f;
#pragma unroll
                for (int t = 0; t < kDescSlots; ++t)
                    if ((unsigned)t < ns) p += ty[t] == tt ? e[t] : 0.f;
                const float g = group_sum<64>(p);
                for (unsigned mm = 0; mm < M; ++mm) {
                    const float *am = s_a + mm * kCmtTrainSlots + lane;
                    float pd = 0.f;
#pragma unroll
                    for (int t = 0; t < kDescSlots; ++t)
                        if ((unsigned)t < ns) pd += ty[t] == tt ? er[t] * am[t * 64] : 0.f;
                    const float gd = group_sum<64>(pd);
                    if (lane == 0) {
                        float *line = s_lines + mm * (kDtLines * 64);
                        line[c] = g;
                        line[64 + c] = gd;
                    }
                }
            }
        }
        __syncthreads();

        // 3. forward, value and tangent: one hidden unit per lane (lanes past the width hold zeros)
        float h1 = 0.f, s1 = 0.f, zd1 = 0.f;
        if ((int)lane < H1) {
            float z1 = b1[lane];
            for (int c = 0; c < D; ++c) {
                const float w = W1[c * ld1 + lane];
                z1 = fmaf(sG[c], w, z1);
                zd1 = fmaf(sGd[c], w, zd1);
            }
            h1 = desc_act<TANH>(z1);
            s1 = TANH ? 1.0f - h1 * h1 : 1.0f;
        }
        lines_publish(sH, sHd, lane, h1, s1 * zd1);
        float h2 = 0.f, s2 = 0.f, zd2 = 0.f, w3 = 0.f;
        if ((int)lane < H2) {
            float z2 = b2[lane];
            for (int c = 0; c < H1; ++c) {
                const float w = W2[c * ld2 + lane];
                z2 = fmaf(sH[c], w, z2);
                zd2 = fmaf(sHd[c], w, zd2);
            }
            h2 = desc_act<TANH>(z2);
            s2 = TANH ? 1.0f - h2 * h2 : 1.0f;
            w3 = W3[lane];
        }

        // 4. reverse over Q = Edot + rho_E E
        const float c2 = TANH ? -2.0f * h2 * s2 : 0.f;
        const float zdb2 = w3 * s2;
        const float zb2 = re * zdb2 + (w3 * c2) * zd2;
        aW3 += fmaf(re, h2, s2 * zd2);
        ab3 += re;
        ab2 += zb2;
        outer_accumulate(aW2, sH, sHd, H1, zb2, zdb2);
        lines_publish(sZ, sZd, lane, zb2, zdb2);
        float zb1 = 0.f, zdb1 = 0.f;
        if ((int)lane < H1) {
            float hb1 = 0.f, hdb1 = 0.f;
            for (int b = 0; b < H2; ++b) {
                const float w = W2[lane * ld2 + b];
                hb1 = fmaf(sZ[b], w, hb1);
                hdb1 = fmaf(sZd[b], w, hdb1);
            }
            const float c1 = TANH ? -2.0f * h1 * s1 : 0.f;
            zdb1 = hdb1 * s1;
            zb1 = hb1 * s1 + (hdb1 * c1) * zd1;
        }
        ab1 += zb1;
        outer_accumulate(aW1, sG, sGd, D, zb1, zdb1);
    }

    // 5. this member's block partial [1 + P], straight from the wave's registers: partials [M][grid][1 + P]
    const int P = (int)dtrain_params((unsigned)D, (unsigned)H1, (unsigned)H2);
    const int oW1 = 1, ob1 = oW1 + D * H1, oW2 = ob1 + H1, ob2 = oW2 + H1 * H2, oW3 = ob2 + H2, ob3 = oW3 + H2;
    float *out = partials + ((size_t)m * gridDim.x + blockIdx.x) * (size_t)(1 + P);
    if ((int)lane < H1) {
#pragma unroll
        for (int c = 0; c < 64; ++c)
            if (c < D) out[oW1 + c * H1 + lane] = aW1[c];
        out[ob1 + lane] = ab1;
    }
    if ((int)lane < H2) {
#pragma unroll
        for (int c = 0; c < 64; ++c)
            if (c < H1) out[oW2 + c * H2 + lane] = aW2[c];
        out[ob2 + lane] = ab2;
        out[oW3 + lane] = aW3;
    }
    if (lane == 0) {
        out[ob3] = ab3;
        out[0] = assr;
    }
}

// accum[m][p] = sum over member m's partials, in a fixed order: a second instance of bp.hip's dtrain_reduce_kernel with the member
// in blockIdx.y, so that all M results take one launch, and sixteen waves to a block instead of four -- wave w adds partials w,
// w + 16, ... for 64 entries, then the sixteen sums are added as a balanced tree.  The gradient entries carry the factor 2 of
// d SSR = 2 sum dQ.  nparts may be 0: the results are then zeros.
__global__ __launch_bounds__(1024) void committee_reduce_kernel(const float *__restrict__ partials, unsigned nparts, unsigned n,
                                                                float *__restrict__ accum, unsigned accum_stride) {
    __shared__ float s[16][64];
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const unsigned p = blockIdx.x * 64u + lane;
    const float *part = partials + (size_t)blockIdx.y * nparts * n;
    float v = 0.f;
    if (p < n)
        for (unsigned g = wave; g < nparts; g += 16) v += part[(size_t)g * n + p];
    s[wave][lane] = v;
    __syncthreads();
    if (wave == 0 && p < n) {
        float t[16];
#pragma unroll
        for (int w = 0; w < 16; ++w) t[w] = s[w][lane];
#pragma unroll
        for (int h = 8; h >= 1; h >>= 1)
#pragma unroll
            for (int w = 0; w < h; ++w) t[w] = t[2 * w] + t[2 * w + 1];
        accum[(size_t)blockIdx.y * accum_stride + p] = p == 0 ? t[0] : 2.0f * t[0];
    }
}

inline unsigned cmt_train_grid(unsigned n, unsigned M) {
    const unsigned g = (n + kCmtTrainRowsPerBlock - 1u) / kCmtTrainRowsPerBlock, cap = kCmtTrainUnits * (kCmtTrainUnitWaves / M);
    return g < cap ? g : cap;
}

inline int cmt_train_check_models(unsigned n_models) {
    HTF_REQUIRE(n_models >= 2 && n_models <= (unsigned)kCmtTrainMaxModels, "descriptor network: n_models = %u outside [2, %d]", n_models,
                kCmtTrainMaxModels);
    return HTF_OK;
}

// dynamic LDS of a launch: M networks, the centres, six exchange lines and one row of a per member
inline size_t cmt_train_lds(unsigned M, unsigned K, unsigned T, unsigned H1, unsigned H2) {
    return ((size_t)M * (cmt_train_lds_member((int)(K * T), (int)H1, (int)H2) + kDtLines * 64 + kCmtTrainSlots) + ((K + 3) & ~3u)) * sizeof(float);
}

// a launch above 64 KiB of dynamic LDS needs the kernel's limit raised first
template <typename F>
inline int cmt_train_raise_lds(F kernel, size_t lds) {
    if (lds > 64u * 1024u)
        HTF_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return HTF_OK;
}

} // namespace
} // namespace htf

extern "C" size_t htf_cmt_scratch_floats(unsigned n_rows, unsigned K, unsigned n_types, unsigned H1, unsigned H2, unsigned n_models) {
    using namespace htf;
    if (dtrain_check(K, n_types, H1, H2) != HTF_OK || cmt_train_check_models(n_models) != HTF_OK) return 0;
    return (size_t)cmt_train_grid(n_rows, n_models) * n_models * (1 + (size_t)dtrain_params(K * n_types, H1, H2));
}

extern "C" int htf_cmt_loss_grad(const void *d_nlist, int nlist_dtype, const int *d_index, unsigned B, unsigned NN, unsigned K,
                                 unsigned n_types, unsigned H1, unsigned H2, int activation, const float *d_weights, const float *d_mu,
                                 float gap, const float *d_rho, float *d_accum, float *d_scratch, const int *d_rows, unsigned n_rows,
                                 float r_cut, unsigned n_models, unsigned weight_stride, unsigned accum_stride, htf_stream stream) {
    using namespace htf;
    // (the residual table stands where htf_bp_loss_grad has the labels and the prediction, as in htf_ct_loss_grad)
    int rc = dtrain_check_call(d_nlist, nlist_dtype, B, NN, K, n_types, H1, H2, activation, d_weights, d_mu, gap, d_rho, HTF_F32, d_rho,
                               d_accum, d_scratch);
    if (rc != HTF_OK) return rc;
    HTF_REQUIRE(B == 0 || d_index, "descriptor network: null pointer");
    if ((rc = desc_check_rows(B, n_rows, r_cut)) != HTF_OK) return rc;
    if ((rc = cmt_train_check_models(n_models)) != HTF_OK) return rc;
    const unsigned P = dtrain_params(K * n_types, H1, H2), n = 1u + P;
    HTF_REQUIRE(weight_stride >= P, "descriptor network: member stride %u below the %u floats of one network", weight_stride, P);
    HTF_REQUIRE(accum_stride >= n, "descriptor network: result stride %u below the %u floats of one member's result", accum_stride, n);
    const size_t lds = cmt_train_lds(n_models, K, n_types, H1, H2);
    HTF_REQUIRE(lds <= (size_t)HTF_CMT_MAX_LDS_BYTES,
                "descriptor network: the training sweep of a committee of %u networks needs %zu bytes of LDS, above the %u bytes of "
                "one compute unit", n_models, lds, HTF_CMT_MAX_LDS_BYTES);
    if (!d_accum) return HTF_OK;   // (B = 0 and nothing to zero-fill: no launch)
    const unsigned grid = cmt_train_grid(n_rows, n_models);   // (0 for no rows: the reductions alone then write zeros)
    const hipStream_t s = (hipStream_t)stream;
    if (grid) {
        dispatch_flags([&](auto TANH, auto CUT, auto LIST, auto F64) {
            using IT = scalar_t<F64>;
            if ((rc = cmt_train_raise_lds(committee_train_kernel<TANH, CUT, LIST, IT>, lds)) != HTF_OK) return;
            hipLaunchKernelGGL((committee_train_kernel<TANH, CUT, LIST, IT>), dim3(grid), dim3(64 * n_models), lds, s,
                               (const typename Vec4<IT>::type *)d_nlist, d_index, d_rows, n_rows, B, NN, d_weights, weight_stride, d_mu,
                               (int)K, (int)n_types, (int)H1, (int)H2, gap, r_cut, (const float4 *)d_rho, d_scratch);
        }, activation == HTF_ACT_TANH, r_cut > 0.0f, d_rows != nullptr, nlist_dtype == HTF_F64);
        if (rc != HTF_OK) return rc;
        const int rl = check_launch("committee_train_kernel");
        if (rl != HTF_OK) return rl;
    }
    // member m's partials are contiguous, [grid][1 + P]: one launch adds them for every member
    hipLaunchKernelGGL(committee_reduce_kernel, dim3((n + 63u) / 64u, n_models), dim3(1024), 0, s, d_scratch, grid, n, d_accum,
                       accum_stride);
    return check_launch("committee_reduce_kernel");
}
