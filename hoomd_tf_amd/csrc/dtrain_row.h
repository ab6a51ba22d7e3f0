// The force-matching sweep's rows (bp.hip, include/htf_bp.h).
//
// With the residual rho_i held fixed, d SSR / d theta = 2 sum_i d Q_i / d theta, Q_i = rho_i . F_i + rho_iE E_i, and
// rho_i . F_i = grad_G E . Gdot is the network's derivative along Gdot_c = sum_j e_k'(r_ij) a_ij, a_ij = 2 (rho_i . t_ij) / r_ij.
// So a row needs one forward pass that carries (value, tangent) through the two hidden layers and one reverse pass over Q:
//
//   z1 = W1^T G + b1, h1 = act(z1), s1 = act'(z1), zd1 = W1^T Gdot, hd1 = s1 zd1        (layer 2 alike; Edot = w3 . hd2)
//   dQ/dw3 = hd2 + rho_E h2, dQ/db3 = rho_E;  zb2 = rho_E w3 s2 + w3 c2 zd2, zdb2 = w3 s2              (c = act'')
//   dQ/dW2 = h1 zb2^T + hd1 zdb2^T, dQ/db2 = zb2;  hb1 = W2 zb2, hdb1 = W2 zdb2
//   zb1 = hb1 s1 + hdb1 c1 zd1, zdb1 = hdb1 s1;  dQ/dW1 = G zb1^T + Gdot zdb1^T, dQ/db1 = zb1
//
// Layout: that of desc_row.h, whose slot reader (desc_slot) the row uses.  One wave64 per row in a grid-stride loop, up to four slots of the row per lane in registers,
// channel t*K + k in lane t*K + k, one hidden unit per lane, activations exchanged through wave-private LDS lines, the
// weights staged in LDS once per block with odd row strides.  G and Gdot are formed together from the same exponentials.
// The weight gradient is kept as outer-product accumulators in registers for the whole kernel: lane a owns column a of dW1
// (64 registers, rows past D stay zero), lane b owns column b of dW2 (64 registers), and one register each for db1, db2,
// dW3, db3 and the loss.  Their loops are unrolled to 64 so every index is a compile-time constant; a block of 16 rows
// past D (past H1) is skipped by a wave-uniform branch.
//
// No atomics and no memset: at the end the four waves of a block add their accumulators in wave order into the LDS that
// held the weights, the block writes one partial [1 + P] to the scratch buffer, and dtrain_reduce_kernel (bp.hip)
// adds the partials in a fixed order into accum.  The grid is a function of the number of work items alone, so two calls
// on the same inputs give the same bits.
//
// Two compile-time switches beside the activation (desc_row.h has the same two):
//   CUT   e_k -> fc(r) e_k, so e_k' a -> (c_der d fc + fc') e_k a; a slot at r >= rc is dropped where the slots are read.
//   LIST  wave work item q handles row rows[q] instead of row q: the labels and the prediction are read at the row, and q
//         alone decides which wave and block accumulate it -- entry q is treated as row q of a batch of n.
// and one of its own:
//   TOTAL the sweep of the conservative forces (ctrain.hip, include/htf_ctrain.h): rho_i . F_i with F = -d(sum E)/dr regroups,
//         row by row, into the same directional derivative with a_ij = ((rho_i - rho_j) . t_ij) / r_ij, j = index[i][slot]
//         (no rho_j for j outside [0, B)).  `pred` is then the residual table rho [B][4], read where the labels and the
//         prediction were; a live slot reads its index and gathers rho_j as one float4, folded into a at once.
#ifndef HTF_DTRAIN_ROW_H_
#define HTF_DTRAIN_ROW_H_
#include "desc_row.h"   // the limits, the activation and the weights' LDS layout are the evaluator's

namespace htf {
namespace {

constexpr int kDtLines = 6;    // exchange lines per wave: G, Gdot, h1, hd1, zb2, zdb2
constexpr unsigned kDtMaxBlocks = 512;   // partials the second kernel adds; each block stages the weights once
constexpr unsigned kDtRowsPerBlock = 64; // rows a block takes before the grid grows: 16 per wave

// two exchange lines at once: every lane's writes are visible to every lane of the wave before the next read
__device__ __forceinline__ void lines_publish(float *la, float *lb, unsigned lane, float a, float b) {
    __builtin_amdgcn_wave_barrier();   // (the previous contents have been read by every lane)
    la[lane] = a;
    lb[lane] = b;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__host__ __device__ inline unsigned dtrain_params(unsigned D, unsigned H1, unsigned H2) { return D * H1 + H1 + H1 * H2 + H2 + H2 + 1; }

// acc[i] += va[i] * ca + vb[i] * cb for the 64 entries of two exchange lines; blocks of 16 past n are skipped (wave-uniform)
__device__ __forceinline__ void outer_accumulate(float (&acc)[64], const float *la, const float *lb, int n, float ca, float cb) {
#pragma unroll
    for (int i0 = 0; i0 < 64; i0 += 16) {
        if (i0 < n) {
#pragma unroll
            for (int i = i0; i < i0 + 16; i += 4) {
                const float4 va = *(const float4 *)(la + i), vb = *(const float4 *)(lb + i);
                acc[i + 0] = fmaf(va.x, ca, fmaf(vb.x, cb, acc[i + 0]));
                acc[i + 1] = fmaf(va.y, ca, fmaf(vb.y, cb, acc[i + 1]));
                acc[i + 2] = fmaf(va.z, ca, fmaf(vb.z, cb, acc[i + 2]));
                acc[i + 3] = fmaf(va.w, ca, fmaf(vb.w, cb, acc[i + 3]));
            }
        }
    }
}

// n work items: rows 0 .. n - 1, or rows[0 .. n - 1] with LIST (rows is then not null); one partial [1 + P] per block
template <bool TANH, bool CUT, bool LIST, typename IT, bool TOTAL = false>
__device__ __forceinline__ void dtrain_rows(const typename Vec4<IT>::type *__restrict__ nlist, const int *__restrict__ rows, unsigned n,
                                            unsigned NN, const float *__restrict__ weights, const float *__restrict__ mu, int K, int T,
                                            int H1, int H2, float gap, float rc, const void *__restrict__ labels, int labels_f64,
                                            const float4 *__restrict__ pred, float *__restrict__ partials,
                                            const int *__restrict__ index = nullptr, unsigned B = 0) {
    extern __shared__ float s_mem[];
    const int D = K * T;
    const int ld1 = H1 + 1, ld2 = H2 + 1;   // odd row strides: a column walk (lane a reads W2[a][b]) spreads over the banks
    const int nw = desc_lds_weights(D, H1, H2);
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    float *s_w = s_mem;
    float *s_mu = s_w + ((nw + 3) & ~3);
    float *s_x = s_mu + ((K + 3) & ~3) + wave * (kDtLines * 64); // this wave's exchange lines
    float *sG = s_x, *sGd = s_x + 64, *sH = s_x + 128, *sHd = s_x + 192, *sZ = s_x + 256, *sZd = s_x + 320;
    float *W1 = s_w, *b1 = W1 + D * ld1, *W2 = b1 + H1, *b2 = W2 + H1 * ld2, *W3 = b2 + H2;
    {
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
    const unsigned ns = (NN + 63u) >> 6;            // slots per lane in use (wave-uniform)
    const unsigned stride = gridDim.x * (blockDim.x >> 6);

    // this wave's share of the gradient: aW1[c] = dW1[c][lane], aW2[a] = dW2[a][lane]
    float aW1[64], aW2[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) aW1[i] = aW2[i] = 0.f;
    float ab1 = 0.f, ab2 = 0.f, aW3 = 0.f, ab3 = 0.f, assr = 0.f;

    for (unsigned q = blockIdx.x * (blockDim.x >> 6) + wave; q < n; q += stride) { // wave-uniform
        unsigned row = q;
        if constexpr (LIST) row = (unsigned)rows[q];
        // 0. the residual (the same value in every lane)
        const float4 pr = pred[row];
        float lx = 0.f, ly = 0.f, lz = 0.f, lw = 0.f;   // (TOTAL: pred is the residual itself)
        if constexpr (!TOTAL) {
            if (labels_f64) {
                const double *lp = (const double *)labels + (size_t)row * 4;
                lx = (float)lp[0]; ly = (float)lp[1]; lz = (float)lp[2]; lw = (float)lp[3];
            } else {
                const float *lp = (const float *)labels + (size_t)row * 4;
                lx = lp[0]; ly = lp[1]; lz = lp[2]; lw = lp[3];
            }
        }
        const float rx = pr.x - lx, ry = pr.y - ly, rz = pr.z - lz, re = pr.w - lw;
        assr += (rx * rx + ry * ry) + (rz * rz + re * re);

        // 1. this lane's slots: distance, type (-1: contributes nothing), a = 2 (rho . t) / r (TOTAL: ((rho - rho_j) . t) / r)
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
                    if constexpr (TOTAL) {
                        float ax = rx, ay = ry, az = rz;
                        const int j = index[(size_t)row * NN + slot];
                        if ((unsigned)j < B) {   // (a negative index is above B as unsigned)
                            const float4 rj = pred[j];
                            ax -= rj.x; ay -= rj.y; az -= rj.z;
                        }
                        a[t] = (ax * s.tx + ay * s.tyy + az * s.tz) / s.rr;
                    } else {
                        a[t] = 2.0f * (rx * s.tx + ry * s.tyy + rz * s.tz) / s.rr;
                    }
                    if constexpr (CUT) cutoff_terms(s.rr, rc, c_fc, fc[t], dfc[t]);
                }
            }
        }

        // 2. G and Gdot from the same exponentials: lane t*K + k ends up holding channel k of type t
        float g_mine = 0.f, gd_mine = 0.f;
        for (int k = 0; k < K; ++k) {
            const float m = s_mu[k];
            float e[kDescSlots], ed[kDescSlots];
#pragma unroll
            for (int t = 0; t < kDescSlots; ++t) {
                e[t] = ed[t] = 0.f;
                if ((unsigned)t < ns) {
                    const float d = r[t] - m;
                    const float ev = __builtin_amdgcn_exp2f(c_exp * (d * d));
                    if constexpr (CUT) {
                        const float el = ty[t] >= 0 ? ev : 0.f;
                        e[t] = fc[t] * el;
                        ed[t] = ((c_der * d) * fc[t] + dfc[t]) * (el * a[t]);
                    } else {
                        e[t] = ty[t] >= 0 ? ev : 0.f;
                        ed[t] = (c_der * d) * (e[t] * a[t]);
                    }
                }
            }
            for (int tt = 0; tt < T; ++tt) {
                float p = 0.f, pd = 0.f;
#pragma unroll
                for (int t = 0; t < kDescSlots; ++t)
                    if ((unsigned)t < ns) {
                        p += ty[t] == tt ? e[t] : 0.f;
                        pd += ty[t] == tt ? ed[t] : 0.f;
                    }
                const float g = group_sum<64>(p), gd = group_sum<64>(pd);
                if ((int)lane == tt * K + k) {
                    g_mine = g;
                    gd_mine = gd;
                }
            }
        }

        // 3. forward, value and tangent: one hidden unit per lane (lanes past the width hold zeros)
        lines_publish(sG, sGd, lane, g_mine, gd_mine);
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

    // 5. the block's partial [1 + P]: the waves add their accumulators, in wave order, into the LDS that held the weights
    const int P = (int)dtrain_params((unsigned)D, (unsigned)H1, (unsigned)H2);
    float *red = s_w;   // (1 + P <= nw)
    const int oW1 = 1, ob1 = oW1 + D * H1, oW2 = ob1 + H1, ob2 = oW2 + H1 * H2, oW3 = ob2 + H2, ob3 = oW3 + H2;
    __syncthreads();    // (every wave has finished reading the weights)
    for (unsigned w = 0; w < (blockDim.x >> 6); ++w) {
        if (wave == w) {
            const bool first = w == 0;
            if ((int)lane < H1) {
#pragma unroll
                for (int c = 0; c < 64; ++c)
                    if (c < D) red[oW1 + c * H1 + lane] = first ? aW1[c] : red[oW1 + c * H1 + lane] + aW1[c];
                red[ob1 + lane] = first ? ab1 : red[ob1 + lane] + ab1;
            }
            if ((int)lane < H2) {
#pragma unroll
                for (int c = 0; c < 64; ++c)
                    if (c < H1) red[oW2 + c * H2 + lane] = first ? aW2[c] : red[oW2 + c * H2 + lane] + aW2[c];
                red[ob2 + lane] = first ? ab2 : red[ob2 + lane] + ab2;
                red[oW3 + lane] = first ? aW3 : red[oW3 + lane] + aW3;
            }
            if (lane == 0) {
                red[ob3] = first ? ab3 : red[ob3] + ab3;
                red[0] = first ? assr : red[0] + assr;
            }
        }
        __syncthreads();
    }
    float *out = partials + (size_t)blockIdx.x * (1 + P);
    for (int i = threadIdx.x; i < 1 + P; i += blockDim.x) out[i] = red[i];
}

inline unsigned dtrain_grid(unsigned n) {
    const unsigned g = (n + kDtRowsPerBlock - 1u) / kDtRowsPerBlock;
    return g < kDtMaxBlocks ? g : kDtMaxBlocks;
}

inline int dtrain_check(unsigned K, unsigned T, unsigned H1, unsigned H2) {
    HTF_REQUIRE(K >= 2 && T >= 1 && K * T <= (unsigned)kDescMaxD && K <= (unsigned)kDescMaxD && T <= (unsigned)kDescMaxD,
                "descriptor network: K = %u, n_types = %u outside 2 <= K, K * n_types <= %d", K, T, kDescMaxD);
    HTF_REQUIRE(H1 >= 1 && H1 <= (unsigned)kDescMaxH && H2 >= 1 && H2 <= (unsigned)kDescMaxH,
                "descriptor network: hidden widths %u, %u outside [1, %d]", H1, H2, kDescMaxH);
    return HTF_OK;
}

// what htf_bp_loss_grad checks of everything but the row list and the cutoff
inline int dtrain_check_call(const void *nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned T, unsigned H1,
                             unsigned H2, int activation, const float *weights, const float *mu, float gap, const void *labels,
                             int labels_dtype, const float *pred, const float *accum, const float *scratch) {
    HTF_REQUIRE(mu && weights && (B == 0 || (nlist && labels && pred && accum && scratch)), "descriptor network: null pointer");
    HTF_REQUIRE(nlist_dtype == HTF_F32 || nlist_dtype == HTF_F64, "descriptor network: unknown nlist dtype %d", nlist_dtype);
    HTF_REQUIRE(labels_dtype == HTF_F32 || labels_dtype == HTF_F64, "descriptor network: unknown labels dtype %d", labels_dtype);
    const int rc = dtrain_check(K, T, H1, H2);
    if (rc != HTF_OK) return rc;
    HTF_REQUIRE(NN <= 64u * kDescSlots, "descriptor network: NN %u > %d", NN, 64 * kDescSlots);
    HTF_REQUIRE(gap > 0.0f, "descriptor network: the centre spacing must be positive (gap = %g)", (double)gap);
    HTF_REQUIRE(activation == HTF_ACT_LINEAR || activation == HTF_ACT_TANH, "descriptor network: unknown activation %d", activation);
    return HTF_OK;
}

inline size_t dtrain_lds(unsigned K, unsigned T, unsigned H1, unsigned H2) {
    return ((((size_t)desc_lds_weights((int)(K * T), (int)H1, (int)H2) + 3) & ~(size_t)3) + ((K + 3) & ~3u) + 4 * kDtLines * 64) * sizeof(float);
}

} // namespace
} // namespace htf
#endif // HTF_DTRAIN_ROW_H_
