// A committee of descriptor networks (include/htf_committee.h, htf.DescriptorMLP(conservative=True, n_models=M)): the mean-model
// conservative forces and the per-particle deviation of M networks, in the two sweeps of cforce.hip.
//
// What dominates a row of those sweeps does not depend on the weights: the slot reads, the NN K exponentials of G_i, the same
// exponentials again in pass 2, the pair tensor and the index.  Both kernels do that part once per row and only the dense
// stack (pass 1) and the gathered runs of g (pass 2) M times.
//
// Pass 1: desc_row.h's row through its step 2 (slots by desc_slot, the same sums in the same order, so G_i is the row
// kernel's), then steps 3 and 4 once per member on the weights of that member, all M networks staged in LDS once
// per block -- two members at a time, one per half of the wave, where the network has at most 32 inputs and hidden units (the
// default widths: a single network leaves those lanes idle).  g[i][m][:] and E_i^m to [B][M][D] and [B][M].
//
// Pass 2: one wave per row, one slot per lane at a time.  The exponential e_k(r) is formed once per slot and centre and used by
// every member; the lane gathers the members' runs g[j][m][t_i K ..] of particle j's one M D-float record (float4 where K is a
// multiple of 4).  The member loops are unrolled to kCmtMaxModels with a wave-uniform break at M, so that every accumulator
// has a compile-time index and lives in a register at every M: no scratch.  F^m and the mean virial follow by the fixed-order
// wave sums, then lane 0 forms the means (pairwise over the members) and the deviations as written: mean first, then the
// differences.  No atomics.  Built with -ffp-contract=on like bp.o and cforce.o (csrc/Makefile).
#include "htf_committee.h"
#include "desc_row.h"

namespace htf {
namespace {

constexpr int kCmtMaxModels = HTF_CMT_MAX_MODELS;
// pass 1 runs 16 waves per block: the M staged networks then serve four times the rows of the family's 256-thread blocks, and
// two blocks of 54 KB (M = 8 at the default widths) fill a compute unit's 32 wave slots where 256-thread blocks left it 8 waves
constexpr int kCmtGradThreads = 1024;

// the sum of kCmtMaxModels values as a balanced tree: three roundings whatever M is (members beyond M are zeros)
__device__ __forceinline__ float cmt_tree_sum(const float (&v)[kCmtMaxModels]) {
    static_assert(kCmtMaxModels == 8, "the tree is written for eight members");
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

// floats of one member's weights in LDS (desc_lds_weights, rounded up to a multiple of 4)
__host__ __device__ inline int cmt_lds_member(int D, int H1, int H2) { return (desc_lds_weights(D, H1, H2) + 3) & ~3; }

// desc_rows' steps 2 to 4 (desc_row.h), statement for statement, as functions: pass 1 runs step 2 once and steps 3 and 4 once per
// member.  desc_rows itself keeps its pasted statements: called from there, these functions moved the scalar-register
// allocation of every bp.o and cforce.o form, and those objects stay what they are.
//
// Step 2: G from the lanes' kept slots (r, fc with CUT, ty; ty = -1 contributes nothing).  Lane t*K + k returns channel k of
// type t, every other lane 0.
template <bool CUT>
__device__ __forceinline__ float cmt_row_channels(const float (&r)[kDescSlots], const float (&fc)[kDescSlots], const int (&ty)[kDescSlots],
                                                  unsigned ns, unsigned lane, const float *s_mu, int K, int T, float c_exp) {
    float g_mine = 0.f;
    for (int k = 0; k < K; ++k) {
        const float m = s_mu[k];
        float e[kDescSlots];
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) e[t] = 0.f;
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) {
            if ((unsigned)t >= ns) break;   // (the wave-uniform branch, as there)
            const float d = r[t] - m;
            const float ev = __builtin_amdgcn_exp2f(c_exp * (d * d));
            if constexpr (CUT)
                e[t] = ty[t] >= 0 ? fc[t] * ev : 0.f;
            else
                e[t] = ty[t] >= 0 ? ev : 0.f;
        }
        for (int tt = 0; tt < T; ++tt) {
            float p = 0.f;
#pragma unroll
            for (int t = 0; t < kDescSlots; ++t)
                if ((unsigned)t < ns) p += ty[t] == tt ? e[t] : 0.f;
            const float g = group_sum<64>(p);
            if ((int)lane == tt * K + k) g_mine = g;
        }
    }
    return g_mine;
}

// One network's weights from global memory into desc_lds_weights' layout at s_w: rows of H + 1 floats, as desc_rows stages them.
__device__ __forceinline__ void cmt_net_stage(float *s_w, const float *__restrict__ weights, int D, int H1, int H2) {
    const int ld1 = H1 + 1, ld2 = H2 + 1;
    float *W1 = s_w, *b1 = W1 + D * ld1, *W2 = b1 + H1, *b2 = W2 + H1 * ld2;
    const float *g_b1 = weights + D * H1, *g_W2 = g_b1 + H1, *g_b2 = g_W2 + H1 * H2;
    for (int i = threadIdx.x; i < D * H1; i += blockDim.x) W1[(i / H1) * ld1 + i % H1] = weights[i];
    for (int i = threadIdx.x; i < H1 * H2; i += blockDim.x) W2[(i / H2) * ld2 + i % H2] = g_W2[i];
    for (int i = threadIdx.x; i < H1; i += blockDim.x) b1[i] = g_b1[i];
    for (int i = threadIdx.x; i < 2 * H2 + 1; i += blockDim.x) b2[i] = g_b2[i]; // b2 | W3 | b3, contiguous in both
}

// Steps 3 and 4 on the network staged at s_w: forward with one hidden unit per lane, then backward to gG = dE/dG, the energy
// returned; s_x is the wave's exchange line.  A network of at most 32 inputs and hidden units leaves half of the wave idle in
// desc_rows; a committee has a second member for it.  W = 32: lanes [0, 32) run one member and lanes [32, 64) the next, each
// half on its own s_w (a per-lane pointer) and its own half of the line, and lane hb + c holds that member's g_c (hb = 0 or
// 32).  W = 64: the whole wave runs one member, as desc_rows does.  `on`: this lane's half has a member (M odd: the last
// pair's upper half has none).  G is read from the lower half's lanes, where cmt_row_channels left it.  A member's sums are
// the same fmaf chains and the first five steps of the same butterfly at either width: its bits do not depend on W.
template <bool TANH, int W>
__device__ __forceinline__ float cmt_net_grad(const float *s_w, bool on, float *s_x, unsigned lane, float g_mine, int D, int H1,
                                              int H2, float &gG) {
    const int l = (int)(lane & (W - 1)), hb = (int)(lane & (64 - W));
    const int ld1 = H1 + 1, ld2 = H2 + 1;
    const float *W1 = s_w, *b1 = W1 + D * ld1, *W2 = b1 + H1, *b2 = W2 + H1 * ld2, *W3 = b2 + H2, *b3 = W3 + H2;
    line_publish(s_x, lane, g_mine);
    float h1 = 0.f;
    if (on && l < H1) {
        float z1 = b1[l];
        for (int c = 0; c < D; ++c) z1 = fmaf(s_x[c], W1[c * ld1 + l], z1);
        h1 = desc_act<TANH>(z1);
    }
    line_publish(s_x, lane, h1);
    float h2 = 0.f;
    if (on && l < H2) {
        float z2 = b2[l];
        for (int a = 0; a < H1; ++a) z2 = fmaf(s_x[hb + a], W2[a * ld2 + l], z2);
        h2 = desc_act<TANH>(z2);
    }
    const float w3 = on && l < H2 ? W3[l] : 0.f;
    const float energy = group_sum<W>(h2 * w3) + (on ? b3[0] : 0.f);

    const float g2 = TANH ? w3 * (1.0f - h2 * h2) : w3;
    line_publish(s_x, lane, g2);
    float g1 = 0.f;
    if (on && l < H1) {
        float acc = 0.f;
        for (int b = 0; b < H2; ++b) acc = fmaf(s_x[hb + b], W2[l * ld2 + b], acc);
        g1 = TANH ? acc * (1.0f - h1 * h1) : acc;
    }
    line_publish(s_x, lane, g1);
    gG = 0.f;
    if (on && l < D) {
        for (int a = 0; a < H1; ++a) gG = fmaf(s_x[hb + a], W1[l * ld1 + a], gG);
    }
    return energy;
}

template <bool TANH, bool CUT, bool LIST, typename IT>
__global__ __launch_bounds__(kCmtGradThreads) void cmt_grad_kernel(const typename Vec4<IT>::type *__restrict__ nlist, const int *__restrict__ rows,
                                                       unsigned n, unsigned NN, const float *__restrict__ weights, unsigned w_stride,
                                                       int M, const float *__restrict__ mu, int K, int T, int H1, int H2, float gap,
                                                       float rc, float *__restrict__ g, float *__restrict__ energy) {
    extern __shared__ float s_mem[];
    const int D = K * T;
    const int nwm = cmt_lds_member(D, H1, H2);
    float *s_mu = s_mem + (size_t)M * nwm;
    float *s_x = s_mu + ((K + 3) & ~3) + (threadIdx.x >> 6) * 64; // this wave's exchange line
    for (int m = 0; m < M; ++m) cmt_net_stage(s_mem + (size_t)m * nwm, weights + (size_t)m * w_stride, D, H1, H2);
    for (int i = threadIdx.x; i < K; i += blockDim.x) s_mu[i] = mu[i];
    __syncthreads();

    const float c_exp = -1.4426950408889634f / gap; // exp(-d^2 / gap) = exp2(c_exp d^2)
    const float c_fc = CUT ? cutoff_slope(rc) : 0.f;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned ns = (NN + 63u) >> 6;            // slots per lane in use (wave-uniform)
    const unsigned stride = gridDim.x * (blockDim.x >> 6);

    for (unsigned q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); q < n; q += stride) { // wave-uniform
        unsigned row = q;
        if constexpr (LIST) row = (unsigned)rows[q];
        const typename Vec4<IT>::type *rp = nlist + (size_t)row * NN;

        // 1. this lane's slots, with the keep rule of desc_rows' step 1
        float r[kDescSlots], fc[kDescSlots];
        int ty[kDescSlots];
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) {
            const unsigned slot = t * 64 + lane;
            r[t] = 1.f;
            fc[t] = 0.f;
            ty[t] = -1;
            if ((unsigned)t < ns && slot < NN) {
                const DescSlot s = desc_slot<IT>(&rp[slot], T);
                bool live = s.rr > kRinvDelta && s.typ >= 0;
                if constexpr (CUT) live = live && s.rr < rc;
                if (live) {
                    r[t] = s.rr;
                    ty[t] = s.typ;
                    if constexpr (CUT) {
                        float dfc;
                        cutoff_terms(s.rr, rc, c_fc, fc[t], dfc);
                    }
                }
            }
        }

        // 2. G, once for all members, by the row kernel's own sums
        const float g_mine = cmt_row_channels<CUT>(r, fc, ty, ns, lane, s_mu, K, T, c_exp);

        // 3, 4. every member's forward and backward on that G: two members at a time where a network fits half a wave
        if (D <= 32 && H1 <= 32 && H2 <= 32) {   // wave-uniform
            for (int m0 = 0; m0 < M; m0 += 2) {
                const int m = m0 + (int)(lane >> 5);
                const bool on = m < M;
                float gG;
                const float e_m = cmt_net_grad<TANH, 32>(s_mem + (size_t)(on ? m : m0) * nwm, on, s_x, lane, g_mine, D, H1, H2, gG);
                if (on && (int)(lane & 31u) < D) g[((size_t)row * M + m) * D + (lane & 31u)] = gG;
                if (on && (lane & 31u) == 0) energy[(size_t)row * M + m] = e_m;
            }
        } else {
            for (int m = 0; m < M; ++m) {
                float gG;
                const float e_m = cmt_net_grad<TANH, 64>(s_mem + (size_t)m * nwm, true, s_x, lane, g_mine, D, H1, H2, gG);
                if ((int)lane < D) g[((size_t)row * M + m) * D + lane] = gG;
                if (lane == 0) energy[(size_t)row * M + m] = e_m;
            }
        }
    }
}

// WIDE: K % 4 == 0 and g is 16-byte aligned (the launcher checks both): a member's run of g is read as K / 4 float4.
template <bool VIRIAL, bool CUT, bool WIDE, typename IT>
__global__ __launch_bounds__(256) void cmt_force_kernel(const typename Vec4<IT>::type *__restrict__ nlist, const int *__restrict__ index,
                                                        const float *__restrict__ types, unsigned B, unsigned NN,
                                                        const float *__restrict__ mu, int K, int T, int M, float gap, float rc,
                                                        const float *__restrict__ g, const float *__restrict__ energy,
                                                        void *__restrict__ out, int out_f64, void *__restrict__ virial9,
                                                        float *__restrict__ dev, float *__restrict__ members) {
    extern __shared__ float s_mem[];
    constexpr int KV = WIDE ? 4 : 1;
    const int D = K * T;
    float *s_mu = s_mem;
    float *s_g = s_mu + ((K + 3) & ~3) + (threadIdx.x >> 6) * (M * 64); // this wave's M lines: its own g_i^m
    for (int i = threadIdx.x; i < K; i += blockDim.x) s_mu[i] = mu[i];
    __syncthreads();

    const float c_exp = -1.4426950408889634f / gap; // exp(-d^2 / gap) = exp2(c_exp d^2)
    const float c_der = -2.0f / gap;                // d e / d r = c_der (r - mu) e
    const float c_fc = CUT ? cutoff_slope(rc) : 0.f;
    const float inv_m = 1.0f / (float)M;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned ns = (NN + 63u) >> 6;            // slots per lane in use (wave-uniform)
    const unsigned stride = gridDim.x * (blockDim.x >> 6);
    const size_t rec = (size_t)M * D;               // floats of one particle's record of g

    for (unsigned row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); row < B; row += stride) { // wave-uniform
        const typename Vec4<IT>::type *rp = nlist + (size_t)row * NN;
        const int *ip = index + (size_t)row * NN;

        // the row's own type (cf_pair_force_kernel's rule) and its own g_i^m, one line per member
        int ti = 0;
        if (T > 1) {
            const float tw = rintf(types[row]);
            ti = (tw >= 0.f && tw < (float)T) ? (int)tw : -1; // (NaN: -1)
        }
        __builtin_amdgcn_wave_barrier();   // (the previous row's lines have been read by every lane)
        for (int m = 0; m < M; ++m) s_g[m * 64 + lane] = (int)lane < D ? g[(size_t)row * rec + m * D + lane] : 0.f;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();

        float fx[kCmtMaxModels], fy[kCmtMaxModels], fz[kCmtMaxModels];
#pragma unroll
        for (int m = 0; m < kCmtMaxModels; ++m) fx[m] = fy[m] = fz[m] = 0.f;
        float w[9];
#pragma unroll
        for (int c9 = 0; c9 < 9; ++c9) w[c9] = 0.f;

        for (unsigned t = 0; t < ns; ++t) {   // wave-uniform: one slot per lane at a time, in slot order
            const unsigned slot = t * 64 + lane;
            // 1. the slot by desc_row.h's desc_slot and cf_pair_force_kernel's keep rule: kept (near) on its distance alone; a
            //    neighbor type outside [0, T) only empties its forward term (ty = -1)
            float x = 0.f, y = 0.f, z = 0.f, r = 1.f, fc = 0.f, dfc = 0.f;
            int ty = -1;
            bool near = false;
            if (slot < NN) {
                const DescSlot s = desc_slot<IT>(&rp[slot], T);
                x = s.x; y = s.y; z = s.z;
                bool live = s.rr > kRinvDelta;
                if constexpr (CUT) live = live && s.rr < rc;
                if (live) {
                    near = true;
                    r = s.rr;
                    ty = s.typ;
                    if constexpr (CUT) cutoff_terms(s.rr, rc, c_fc, fc, dfc);
                }
            }
            // 2. where the slot's reverse terms live: the record of particle j at its run t_i K, or nowhere
            const float *gj = nullptr;
            if (near && ti >= 0) {   // (a kept slot: slot < NN)
                const int j = ip[slot];
                if ((unsigned)j < B) gj = g + ((size_t)j * rec + ti * K);
            }
            const float *gi = s_g + (ty > 0 ? ty : 0) * K;

            // 3. dE^m_total/dr of the slot for every member, each exponential formed once
            float acc[kCmtMaxModels], acc0[kCmtMaxModels];
#pragma unroll
            for (int m = 0; m < kCmtMaxModels; ++m) acc[m] = acc0[m] = 0.f;
            for (int k0 = 0; k0 < K; k0 += KV) {
                float de[KV], ev[KV];   // (r - mu_k) e_k and e_k
#pragma unroll
                for (int kk = 0; kk < KV; ++kk) {
                    const float d = r - s_mu[k0 + kk];
                    ev[kk] = __builtin_amdgcn_exp2f(c_exp * (d * d));
                    de[kk] = d * ev[kk];
                }
#pragma unroll
                for (int m = 0; m < kCmtMaxModels; ++m) {
                    if (m >= M) break;   // wave-uniform
                    float gr[KV];
#pragma unroll
                    for (int kk = 0; kk < KV; ++kk) gr[kk] = 0.f;
                    if (gj != nullptr) {
                        if constexpr (WIDE) {
                            const float4 v = *reinterpret_cast<const float4 *>(gj + m * D + k0);
                            gr[0] = v.x; gr[1] = v.y; gr[2] = v.z; gr[3] = v.w;
                        } else {
                            gr[0] = gj[m * D + k0];
                        }
                    }
#pragma unroll
                    for (int kk = 0; kk < KV; ++kk) {
                        const float own = gi[m * 64 + k0 + kk];
                        const float gk = (ty >= 0 ? own : 0.f) + gr[kk];
                        acc[m] = fmaf(gk, de[kk], acc[m]);
                        if constexpr (CUT) acc0[m] = fmaf(gk, ev[kk], acc0[m]);
                    }
                }
            }

            // 4. phi^m of the slot into F^m, and the members' mean into the mean virial
            if (near) {
                const float tx = x + kNormDelta, tyy = y + kNormDelta, tz = z + kNormDelta;
                float cs = 0.f;
#pragma unroll
                for (int m = 0; m < kCmtMaxModels; ++m) {
                    if (m >= M) break;
                    float c;
                    if constexpr (CUT)
                        c = (fc * (c_der * acc[m]) + dfc * acc0[m]) / r;
                    else
                        c = (c_der * acc[m]) / r;
                    fx[m] += c * tx; fy[m] += c * tyy; fz[m] += c * tz;
                    cs += c;
                }
                if constexpr (VIRIAL) {
                    const float cb = cs * inv_m;
                    const float ax = cb * tx, ay = cb * tyy, az = cb * tz;
                    const float hx = -0.5f * x, hy = -0.5f * y, hz = -0.5f * z;
                    w[0] += hx * ax; w[1] += hx * ay; w[2] += hx * az;
                    w[3] += hy * ax; w[4] += hy * ay; w[5] += hy * az;
                    w[6] += hz * ax; w[7] += hz * ay; w[8] += hz * az;
                }
            }
        }

        // 5. the fixed-order wave sums, then lane 0: means, deviations (mean first, then the differences) and the stores
#pragma unroll
        for (int m = 0; m < kCmtMaxModels; ++m) {
            if (m >= M) break;
            fx[m] = group_sum<64>(fx[m]);
            fy[m] = group_sum<64>(fy[m]);
            fz[m] = group_sum<64>(fz[m]);
        }
        if constexpr (VIRIAL) {
#pragma unroll
            for (int c9 = 0; c9 < 9; ++c9) w[c9] = group_sum<64>(w[c9]);
        }
        if (lane == 0) {
            float e[kCmtMaxModels];
#pragma unroll
            for (int m = 0; m < kCmtMaxModels; ++m) e[m] = m < M ? energy[(size_t)row * M + m] : 0.f;
            const float mx = cmt_tree_sum(fx) / (float)M, my = cmt_tree_sum(fy) / (float)M, mz = cmt_tree_sum(fz) / (float)M;
            const float me = cmt_tree_sum(e) / (float)M;
            float df[kCmtMaxModels], de[kCmtMaxModels];
#pragma unroll
            for (int m = 0; m < kCmtMaxModels; ++m) {
                const float dx = fx[m] - mx, dy = fy[m] - my, dz = fz[m] - mz, dd = e[m] - me;
                df[m] = m < M ? dx * dx + dy * dy + dz * dz : 0.f;
                de[m] = m < M ? dd * dd : 0.f;
            }
            dev[(size_t)row * 2] = sqrtf(cmt_tree_sum(df) / (float)M);
            dev[(size_t)row * 2 + 1] = sqrtf(cmt_tree_sum(de) / (float)M);
            if (out_f64)
                ((double4 *)out)[row] = make_double4(mx, my, mz, me);
            else
                ((float4 *)out)[row] = make_float4(mx, my, mz, me);
            if constexpr (VIRIAL) {
#pragma unroll
                for (int c9 = 0; c9 < 9; ++c9) {
                    if (out_f64)
                        ((double *)virial9)[(size_t)row * 9 + c9] = w[c9];
                    else
                        ((float *)virial9)[(size_t)row * 9 + c9] = w[c9];
                }
            }
            if (members != nullptr) {
#pragma unroll
                for (int m = 0; m < kCmtMaxModels; ++m) {
                    if (m >= M) break;
                    ((float4 *)members)[(size_t)m * B + row] = make_float4(fx[m], fy[m], fz[m], e[m]);
                }
            }
        }
    }
}

inline int cmt_check_models(unsigned n_models) {
    HTF_REQUIRE(n_models >= 2 && n_models <= (unsigned)kCmtMaxModels, "descriptor network: n_models = %u outside [2, %d]", n_models,
                kCmtMaxModels);
    return HTF_OK;
}

// dynamic LDS of a pass-1 launch (M networks, centres, one exchange line per wave) and of a pass-2 launch (centres, M lines per wave)
inline size_t cmt_lds_grad(unsigned M, unsigned K, unsigned T, unsigned H1, unsigned H2) {
    return ((size_t)M * cmt_lds_member((int)(K * T), (int)H1, (int)H2) + ((K + 3) & ~3u) + kCmtGradThreads) * sizeof(float);
}
inline unsigned cmt_grid_grad(unsigned n) {
    const unsigned g = (n + kCmtGradThreads / 64 - 1) / (kCmtGradThreads / 64);
    return g < kDescMaxBlocks ? g : kDescMaxBlocks;
}
inline size_t cmt_lds_forces(unsigned M, unsigned K) { return (((K + 3) & ~3u) + 4 * (size_t)M * 64) * sizeof(float); }

// a launch above 64 KiB of dynamic LDS needs the kernel's limit raised first
template <typename F>
inline int cmt_raise_lds(F kernel, size_t lds) {
    if (lds > 64u * 1024u)
        HTF_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return HTF_OK;
}

} // namespace
} // namespace htf

extern "C" int htf_cmt_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types, unsigned H1,
                            unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap, float *d_g,
                            float *d_energy, const int *d_rows, unsigned n_rows, float r_cut, unsigned n_models,
                            unsigned weight_stride, htf_stream stream) {
    using namespace htf;
    int rc = desc_check(d_nlist, nlist_dtype, B, NN, K, n_types, d_mu, gap, d_g, HTF_F32);
    if (rc != HTF_OK) return rc;
    if ((rc = desc_check_network(d_weights, H1, H2, activation)) != HTF_OK) return rc;
    if ((rc = desc_check_rows(B, n_rows, r_cut)) != HTF_OK) return rc;
    if ((rc = cmt_check_models(n_models)) != HTF_OK) return rc;
    const unsigned D = K * n_types, P = D * H1 + H1 + H1 * H2 + H2 + H2 + 1;
    HTF_REQUIRE(weight_stride >= P, "descriptor network: member stride %u below the %u floats of one network", weight_stride, P);
    HTF_REQUIRE(B == 0 || d_energy, "descriptor network: null pointer");
    const size_t lds = cmt_lds_grad(n_models, K, n_types, H1, H2);
    HTF_REQUIRE(lds <= (size_t)HTF_CMT_MAX_LDS_BYTES,
                "descriptor network: a committee of %u networks needs %zu bytes of LDS, above the %u bytes of one compute unit",
                n_models, lds, HTF_CMT_MAX_LDS_BYTES);
    if (n_rows == 0) return HTF_OK;
    const hipStream_t s = (hipStream_t)stream;
    dispatch_flags([&](auto TANH, auto CUT, auto LIST, auto F64) {
        using IT = scalar_t<F64>;
        if ((rc = cmt_raise_lds(cmt_grad_kernel<TANH, CUT, LIST, IT>, lds)) != HTF_OK) return;
        hipLaunchKernelGGL((cmt_grad_kernel<TANH, CUT, LIST, IT>), dim3(cmt_grid_grad(n_rows)), dim3(kCmtGradThreads), lds, s,
                           (const typename Vec4<IT>::type *)d_nlist, d_rows, n_rows, NN, d_weights, weight_stride, (int)n_models, d_mu,
                           (int)K, (int)n_types, (int)H1, (int)H2, gap, r_cut, d_g, d_energy);
    }, activation == HTF_ACT_TANH, r_cut > 0.0f, d_rows != nullptr, nlist_dtype == HTF_F64);
    if (rc != HTF_OK) return rc;
    return check_launch("cmt_grad_kernel");
}

extern "C" int htf_cmt_forces(const void *d_nlist, int nlist_dtype, const int *d_index, const float *d_types, unsigned B, unsigned NN,
                              unsigned K, unsigned n_types, const float *d_mu, float gap, const float *d_g, const float *d_energy,
                              void *d_force, int force_dtype, void *d_virial9, float r_cut, unsigned n_models, float *d_dev,
                              float *d_members, htf_stream stream) {
    using namespace htf;
    int rc = desc_check(d_nlist, nlist_dtype, B, NN, K, n_types, d_mu, gap, d_force, force_dtype);
    if (rc != HTF_OK) return rc;
    if ((rc = desc_check_rows(B, B, r_cut)) != HTF_OK) return rc;
    if ((rc = cmt_check_models(n_models)) != HTF_OK) return rc;
    HTF_REQUIRE(B == 0 || (d_index && d_g && d_energy && d_dev), "descriptor network: null pointer");
    HTF_REQUIRE(B == 0 || n_types == 1 || d_types, "descriptor network: n_types = %u needs the rows' own types", n_types);
    if (B == 0) return HTF_OK;
    const size_t lds = cmt_lds_forces(n_models, K);
    const int out_f64 = force_dtype == HTF_F64;
    const bool wide = K % 4u == 0 && ((uintptr_t)d_g & 15u) == 0;
    const hipStream_t s = (hipStream_t)stream;
    dispatch_flags([&](auto VIR, auto CUT, auto WIDE, auto F64) {
        using IT = scalar_t<F64>;
        hipLaunchKernelGGL((cmt_force_kernel<VIR, CUT, WIDE, IT>), dim3(desc_grid(B)), dim3(256), lds, s,
                           (const typename Vec4<IT>::type *)d_nlist, d_index, d_types, B, NN, d_mu, (int)K, (int)n_types, (int)n_models,
                           gap, r_cut, d_g, d_energy, d_force, out_f64, d_virial9, d_dev, d_members);
    }, d_virial9 != nullptr, r_cut > 0.0f, wide, nlist_dtype == HTF_F64);
    return check_launch("cmt_force_kernel");
}
