// The descriptor network's rows (bp.hip, include/htf_bp.h): forces, energy and virial, or the descriptor alone.
//
// One wave64 per particle row, the shape of topk_mlp.hip.  Each lane holds up to four slots of the row (NN <= 256) in
// registers: pair vector, distance and type, read once (16 B per slot, 32 B from an fp64 tensor).  Channel k of type t is
// formed as each lane's sum over its own slots (slot order) followed by a wave reduction (fixed DPP butterfly), and lands
// in lane t*K + k.  The network runs with one hidden unit per lane, activations exchanged through a wave-private LDS line
// (broadcast reads): forward, then backward to g_c = dE/dG_c (lane c).  Each lane then forms its own slots' dE/dr from
// dE/dG and d e_k/dr = -2 (r - mu_k) / gap * e_k, and from it the slot's force and virial terms, summed over the wave.
//
// The backward RECOMPUTES e_k: K more exponentials per slot.  Keeping them would take K registers per slot, up to
// 4 * 64 = 256 VGPRs at the limits (past the register file of one lane); recomputing costs none.  Each exponential is one
// v_exp_f32 on the argument -(r - mu)^2 log2(e) / gap; far beyond the last centre it underflows to 0, never to NaN.
//
// No atomics, no scratch, no global intermediate; the weights are staged in LDS once per block (rows padded to an odd
// stride) and every wave walks rows in
// a grid-stride loop.  A row's bits depend on its slots alone, not on the batch, grid or wave that evaluates it, and the
// descriptor-only entry runs the same code for G.  Built with -ffp-contract=on (csrc/Makefile): multiply-adds are fused
// only inside a source expression, so both instantiations (descriptor only, forces) form G identically.
//
// Two compile-time switches beside the outputs:
//   CUT   the cosine cutoff fc(r) = 0.5 (cos(pi r / rc) + 1), r < rc, multiplied into every Gaussian.  A slot at r >= rc is
//         dropped where the slots are read, exactly like a padded one; fc and fc' = -0.5 (pi / rc) sin(pi r / rc) are formed
//         once per slot where its distance is (sincospif: the reduction of r / rc in [0, 1) is exact) and kept, two
//         registers per slot.  dE/dr = fc c_der sum_k g_k d_k e_k + fc' sum_k g_k e_k: a second accumulator per slot.
//   LIST  wave work item q handles row rows[q] instead of row q; the launcher selects it by whether it was given a list.
//         Outputs are indexed by the row.  Without it the row index costs the default route nothing.
#ifndef HTF_DESC_ROW_H_
#define HTF_DESC_ROW_H_
#include "dispatch.h"
#include "htf_common.h"
#include "htf_internal.h"
#include "pair_math.h"
#include "bp_cutoff.h"

namespace htf {
namespace {

constexpr int kDescMaxD = 64;   // channels: one per lane
constexpr int kDescMaxH = 64;   // hidden units: one per lane
constexpr int kDescSlots = 4;   // slots per lane: NN <= 256
constexpr unsigned kDescMaxBlocks = 2048; // grid-stride: each block stages the weights once for many rows

template <bool TANH>
__device__ __forceinline__ float desc_act(float z) {
    if constexpr (!TANH) return z;
    return fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * z)), 1.0f);
}

// exchange line: every lane's writes are visible to every lane of the wave before the next read
__device__ __forceinline__ void line_publish(float *line, unsigned lane, float v) {
    __builtin_amdgcn_wave_barrier();   // (the previous contents have been read by every lane)
    line[lane] = v;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// floats of the weights in LDS: W1 [D][H1 + 1] | b1 | W2 [H1][H2 + 1] | b2 | W3 | b3
__host__ __device__ inline int desc_lds_weights(int D, int H1, int H2) { return D * (H1 + 1) + H1 + H1 * (H2 + 1) + H2 + H2 + 1; }

// One slot of a row as every kernel of the family reads it: 16 B (32 B from an fp64 tensor), once.  Which slots a kernel
// keeps is its own rule, written with these fields where the slot is read.  (Returned by value, not filled through a pointer:
// the fields are then plain values before anything is inlined, as the pasted statements' locals were.)
struct DescSlot {
    float x, y, z;      // the raw pair vector (the virial's)
    float tx, tyy, tz;  // shifted by 1e-7 as the graph shifts it (tyy: ty[] is the slots' types wherever a slot is read)
    float rr;           // |t|
    int typ;            // the neighbor's type in [0, T), or -1
};
template <typename IT>
__device__ __forceinline__ DescSlot desc_slot(const typename Vec4<IT>::type *p, int T) {
    const auto v = load_stream(p);
    const float x = (float)v.x, y = (float)v.y, z = (float)v.z;
    const float tx = x + kNormDelta, tyy = y + kNormDelta, tz = z + kNormDelta;
    const float rr = sqrtf(tx * tx + tyy * tyy + tz * tz);
    int typ = 0;
    if (T > 1) {
        const IT rw = rint(v.w);
        typ = (rw >= (IT)0 && rw < (IT)T) ? (int)rw : -1; // (NaN: -1)
    }
    return {x, y, z, tx, tyy, tz, rr, typ};
}

// The end of a pass-2 row of the conservative forces (cforce.hip, angular.hip): the fixed-order wave sums of the lanes' F and W
// terms, then lane 0 stores them, with the row's energy from pass 1, in either output dtype.
template <bool VIRIAL>
__device__ __forceinline__ void desc_pair_force_end(unsigned lane, unsigned row, float fx, float fy, float fz, float (&w)[9],
                                                    const float *__restrict__ energy, void *out, int out_f64, void *virial9) {
    fx = group_sum<64>(fx);
    fy = group_sum<64>(fy);
    fz = group_sum<64>(fz);
    if constexpr (VIRIAL) {
#pragma unroll
        for (int c9 = 0; c9 < 9; ++c9) w[c9] = group_sum<64>(w[c9]);
    }
    if (lane == 0) {
        const float e = energy[row];
        if (out_f64)
            ((double4 *)out)[row] = make_double4(fx, fy, fz, e);
        else
            ((float4 *)out)[row] = make_float4(fx, fy, fz, e);
        if constexpr (VIRIAL) {
#pragma unroll
            for (int c9 = 0; c9 < 9; ++c9) {
                if (out_f64)
                    ((double *)virial9)[(size_t)row * 9 + c9] = w[c9];
                else
                    ((float *)virial9)[(size_t)row * 9 + c9] = w[c9];
            }
        }
    }
}

// FORCES = false: G alone, written to out [B][D].  FORCES = true: out [B][4] (f, E) and, with VIRIAL, virial9 [B][9].
// n work items: rows 0 .. n - 1, or rows[0 .. n - 1] with LIST (rows is then not null).
// GRAD (with FORCES, pass 1 of the conservative forces, cforce.hip): the row ends after step 4 -- out [B][D] fp32 receives
// g = dE/dG from lanes < D and virial9 [B] fp32 the energy, the bits the force instantiation writes.
template <bool FORCES, bool TANH, bool VIRIAL, bool CUT, bool LIST, typename IT, bool GRAD = false>
__device__ __forceinline__ void desc_rows(const typename Vec4<IT>::type *__restrict__ nlist, const int *__restrict__ rows, unsigned n,
                                          unsigned NN, const float *__restrict__ weights, const float *__restrict__ mu, int K, int T,
                                          int H1, int H2, float gap, float rc, void *__restrict__ out, int out_f64,
                                          void *__restrict__ virial9) {
    extern __shared__ float s_mem[];
    const int D = K * T;
    // W1 and W2 are staged with rows of H + 1 floats: the backward reads them down a column (lane c reads W1[c][a]), and an
    // odd row stride puts the 64 lanes' reads in different banks where a stride of 64 would serialise them
    const int ld1 = H1 + 1, ld2 = H2 + 1;
    const int nw = FORCES ? desc_lds_weights(D, H1, H2) : 0;
    float *s_w = s_mem;
    float *s_mu = s_w + ((nw + 3) & ~3);
    float *s_x = s_mu + ((K + 3) & ~3) + (threadIdx.x >> 6) * 64; // this wave's exchange line
    float *W1 = s_w, *b1 = W1 + D * ld1, *W2 = b1 + H1, *b2 = W2 + H1 * ld2, *W3 = b2 + H2, *b3 = W3 + H2;
    if constexpr (FORCES) {
        const float *g_b1 = weights + D * H1, *g_W2 = g_b1 + H1, *g_b2 = g_W2 + H1 * H2;
        for (int i = threadIdx.x; i < D * H1; i += blockDim.x) W1[(i / H1) * ld1 + i % H1] = weights[i];
        for (int i = threadIdx.x; i < H1 * H2; i += blockDim.x) W2[(i / H2) * ld2 + i % H2] = g_W2[i];
        for (int i = threadIdx.x; i < H1; i += blockDim.x) b1[i] = g_b1[i];
        for (int i = threadIdx.x; i < 2 * H2 + 1; i += blockDim.x) b2[i] = g_b2[i]; // b2 | W3 | b3, contiguous in both
    }
    for (int i = threadIdx.x; i < K; i += blockDim.x) s_mu[i] = mu[i];
    __syncthreads();

    const float c_exp = -1.4426950408889634f / gap; // exp(-d^2 / gap) = exp2(c_exp d^2)
    const float c_der = -2.0f / gap;                // d e / d r = c_der (r - mu) e
    const float c_fc = CUT ? cutoff_slope(rc) : 0.f;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned ns = (NN + 63u) >> 6;            // slots per lane in use (wave-uniform)
    const unsigned stride = gridDim.x * (blockDim.x >> 6);

    for (unsigned q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); q < n; q += stride) { // wave-uniform
        unsigned row = q;
        if constexpr (LIST) row = (unsigned)rows[q];
        const typename Vec4<IT>::type *rp = nlist + (size_t)row * NN;

        // 1. this lane's slots: raw pair vector (virial), distance, type (-1: contributes nothing)
        float x[kDescSlots], y[kDescSlots], z[kDescSlots], r[kDescSlots];
        float fc[kDescSlots], dfc[kDescSlots];   // (CUT only)
        int ty[kDescSlots];
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) {
            const unsigned slot = t * 64 + lane;
            x[t] = y[t] = z[t] = 0.f;
            r[t] = 1.f;
            fc[t] = dfc[t] = 0.f;
            ty[t] = -1;
            if ((unsigned)t < ns && slot < NN) {
                const DescSlot s = desc_slot<IT>(&rp[slot], T);
                x[t] = s.x; y[t] = s.y; z[t] = s.z;
                bool live = s.rr > kRinvDelta && s.typ >= 0;
                if constexpr (CUT) live = live && s.rr < rc;
                if (live) {
                    r[t] = s.rr;
                    ty[t] = s.typ;
                    if constexpr (CUT) cutoff_terms(s.rr, rc, c_fc, fc[t], dfc[t]);
                }
            }
        }

        // 2. G: lane t*K + k ends up holding channel k of type t
        float g_mine = 0.f;
        for (int k = 0; k < K; ++k) {
            const float m = s_mu[k];
            float e[kDescSlots];
#pragma unroll
            for (int t = 0; t < kDescSlots; ++t) e[t] = 0.f;
#pragma unroll
            for (int t = 0; t < kDescSlots; ++t) {
                // a break, not `if (t < ns) {...}`: inlined into a kernel that guard was if-converted and all four exponentials ran
                // at every NN; the break keeps the wave-uniform branch, so a row of NN <= 64 t slots pays for t of them
                if ((unsigned)t >= ns) break;
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
        if constexpr (!FORCES) {
            if ((int)lane < D) {
                if (out_f64)
                    ((double *)out)[(size_t)row * D + lane] = g_mine;
                else
                    ((float *)out)[(size_t)row * D + lane] = g_mine;
            }
            continue;
        }

        // 3. forward: one hidden unit per lane
        line_publish(s_x, lane, g_mine);
        float h1 = 0.f;
        if ((int)lane < H1) {
            float z1 = b1[lane];
            for (int c = 0; c < D; ++c) z1 = fmaf(s_x[c], W1[c * ld1 + lane], z1);
            h1 = desc_act<TANH>(z1);
        }
        line_publish(s_x, lane, h1);
        float h2 = 0.f;
        if ((int)lane < H2) {
            float z2 = b2[lane];
            for (int a = 0; a < H1; ++a) z2 = fmaf(s_x[a], W2[a * ld2 + lane], z2);
            h2 = desc_act<TANH>(z2);
        }
        const float w3 = (int)lane < H2 ? W3[lane] : 0.f;
        const float energy = group_sum<64>(h2 * w3) + b3[0];

        // 4. backward: g2 = dE/dz2, g1 = dE/dz1, gG = dE/dG
        const float g2 = TANH ? w3 * (1.0f - h2 * h2) : w3;
        line_publish(s_x, lane, g2);
        float g1 = 0.f;
        if ((int)lane < H1) {
            float acc = 0.f;
            for (int b = 0; b < H2; ++b) acc = fmaf(s_x[b], W2[lane * ld2 + b], acc);
            g1 = TANH ? acc * (1.0f - h1 * h1) : acc;
        }
        line_publish(s_x, lane, g1);
        float gG = 0.f;
        if ((int)lane < D) {
            for (int a = 0; a < H1; ++a) gG = fmaf(s_x[a], W1[lane * ld1 + a], gG);
        }
        if constexpr (GRAD) {
            if ((int)lane < D) ((float *)out)[(size_t)row * D + lane] = gG;
            if (lane == 0) ((float *)virial9)[row] = energy;
            continue;
        }
        line_publish(s_x, lane, gG);

        // 5. every lane: dE/dr of its own slots (exponentials recomputed), then forces and virial
        float acc[kDescSlots], acc0[kDescSlots];   // sum_k g_k d_k e_k and (CUT only) sum_k g_k e_k
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) acc[t] = acc0[t] = 0.f;
        for (int k = 0; k < K; ++k) {
            const float m = s_mu[k];
#pragma unroll
            for (int t = 0; t < kDescSlots; ++t) {
                if ((unsigned)t < ns) {
                    const float d = r[t] - m;
                    const float ev = __builtin_amdgcn_exp2f(c_exp * (d * d));
                    const float gk = s_x[(ty[t] > 0 ? ty[t] : 0) * K + k];
                    acc[t] = fmaf(gk * d, ev, acc[t]);
                    if constexpr (CUT) acc0[t] = fmaf(gk, ev, acc0[t]);
                }
            }
        }
        float fx = 0.f, fy = 0.f, fz = 0.f;
        Virial6 vir;
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) {
            if ((unsigned)t < ns && ty[t] >= 0) {
                // nlist_forces = 2 dE/dx = 2 (dE/dr) (x + 1e-7) / r  (simmodel.py:548)
                float c;
                if constexpr (CUT)
                    c = 2.0f * (fc[t] * (c_der * acc[t]) + dfc[t] * acc0[t]) / r[t];
                else
                    c = 2.0f * (c_der * acc[t]) / r[t];
                const float ax = c * (x[t] + kNormDelta), ay = c * (y[t] + kNormDelta), az = c * (z[t] + kNormDelta);
                fx += ax; fy += ay; fz += az;
                if constexpr (VIRIAL) vir.add(x[t], y[t], z[t], ax, ay, az);
            }
        }
        fx = group_sum<64>(fx);
        fy = group_sum<64>(fy);
        fz = group_sum<64>(fz);
        float v6[6];
        if constexpr (VIRIAL) {
            v6[0] = group_sum<64>(vir.xx); v6[1] = group_sum<64>(vir.xy); v6[2] = group_sum<64>(vir.xz);
            v6[3] = group_sum<64>(vir.yy); v6[4] = group_sum<64>(vir.yz); v6[5] = group_sum<64>(vir.zz);
        }
        if (lane == 0) {
            if (out_f64)
                ((double4 *)out)[row] = make_double4(fx, fy, fz, energy);
            else
                ((float4 *)out)[row] = make_float4(fx, fy, fz, energy);
            if constexpr (VIRIAL) {
                const float v9[9] = {v6[0], v6[1], v6[2], v6[1], v6[3], v6[4], v6[2], v6[4], v6[5]};
#pragma unroll
                for (int c9 = 0; c9 < 9; ++c9) {
                    if (out_f64)
                        ((double *)virial9)[(size_t)row * 9 + c9] = v9[c9];
                    else
                        ((float *)virial9)[(size_t)row * 9 + c9] = v9[c9];
                }
            }
        }
    }
}

inline int desc_check(const void *nlist, int in_dtype, unsigned B, unsigned NN, unsigned K, unsigned T, const float *mu, float gap,
                      const void *out, int out_dtype) {
    HTF_REQUIRE(mu && (B == 0 || (nlist && out)), "descriptor network: null pointer");
    HTF_REQUIRE(in_dtype == HTF_F32 || in_dtype == HTF_F64, "descriptor network: unknown nlist dtype %d", in_dtype);
    HTF_REQUIRE(out_dtype == HTF_F32 || out_dtype == HTF_F64, "descriptor network: unknown output dtype %d", out_dtype);
    HTF_REQUIRE(K >= 2 && T >= 1 && K * T <= (unsigned)kDescMaxD, "descriptor network: K = %u, n_types = %u outside 2 <= K, K * n_types <= %d",
                K, T, kDescMaxD);
    HTF_REQUIRE(NN <= 64u * kDescSlots, "descriptor network: NN %u > %d", NN, 64 * kDescSlots);
    HTF_REQUIRE(gap > 0.0f, "descriptor network: the centre spacing must be positive (gap = %g)", (double)gap);
    return HTF_OK;
}

inline int desc_check_network(const float *weights, unsigned H1, unsigned H2, int activation) {
    HTF_REQUIRE(weights, "descriptor network: null weights");
    HTF_REQUIRE(H1 >= 1 && H1 <= (unsigned)kDescMaxH && H2 >= 1 && H2 <= (unsigned)kDescMaxH,
                "descriptor network: hidden widths %u, %u outside [1, %d]", H1, H2, kDescMaxH);
    HTF_REQUIRE(activation == HTF_ACT_LINEAR || activation == HTF_ACT_TANH, "descriptor network: unknown activation %d", activation);
    return HTF_OK;
}

// a row list and a cutoff as every entry that takes them checks them
inline int desc_check_rows(unsigned B, unsigned n_rows, float r_cut) {
    HTF_REQUIRE(n_rows <= B, "descriptor network: n_rows %u > B %u", n_rows, B);
    HTF_REQUIRE(r_cut >= 0.0f && r_cut <= 3.402823466e+38f, "descriptor network: r_cut = %g must be finite and positive, or 0 for none",
                (double)r_cut);
    return HTF_OK;
}

// dynamic LDS of a forces launch (weights, centres, one exchange line per wave) and of a descriptor-only launch
inline size_t desc_lds_forces(unsigned K, unsigned T, unsigned H1, unsigned H2) {
    return ((((size_t)desc_lds_weights((int)(K * T), (int)H1, (int)H2) + 3) & ~(size_t)3) + ((K + 3) & ~3u) + 4 * 64) * sizeof(float);
}
inline size_t desc_lds_descriptor(unsigned K) { return (((K + 3) & ~3u) + 4 * 64) * sizeof(float); }

inline unsigned desc_grid(unsigned n) {
    const unsigned g = (n + 3u) / 4u;
    return g < kDescMaxBlocks ? g : kDescMaxBlocks;
}

} // namespace
} // namespace htf
#endif // HTF_DESC_ROW_H_
