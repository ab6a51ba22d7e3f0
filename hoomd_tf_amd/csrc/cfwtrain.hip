// Force matching on the conservative forces for wide networks (include/htf_cfwtrain.h, htf.DescriptorMLP.wide_loss_gradient,
// trainable="wide"): ctrain.hip's sweep with the dense stack on v_mfma_f32_32x32x2_f32, hidden layers up to 256 wide.
//
// The mathematics is dtrain_row.h's: a row's forward pass carries (value, tangent) along Gdot, a = ((rho_i - rho_j) . t) / r,
// and one reverse pass runs over Q = Edot + rho_E E.  With hd = s zd the second-derivative terms are c zd = -2 h hd (tanh; 0
// for linear), so every image is a (value, tangent) pair:
//   zb2 = rho_E w3 s2 - 2 w3 h2 hd2, zdb2 = w3 s2;   zb1 = hb1 s1 - 2 h1 hd1 hdb1, zdb1 = hdb1 s1,   s = 1 - h^2.
//
// One block of eight waves works on a tile of 32 listed rows at a time (grid-stride over the tiles) and keeps cfwide.hip's three
// LDS images, one line of 64 floats per feature, lines 65 floats apart -- columns 0..31 of a line the VALUE of the 32 rows,
// columns 32..63 the TANGENT:
//
//   X  [D32 ][65]  (G | Gdot)       A1 [H1p][65]  (h1 | hd1), later (zb1 | zdb1)       A2 [H2p][65]  (zb2 | zdb2)
//
// so that cfwide.hip's cfw_mm with two accumulators (copied below statement for statement) feeds every weight it reads from L2
// to one value and one tangent instruction, forward and backward access patterns as there.  Phases of a tile, a block barrier
// between them:
//   1. descriptor   the waves split the rows; a row is dtrain_rows' steps 0 to 2 with TOTAL (the residual, the slots with the
//                   gathered rho_j, G and Gdot from the same exponentials); rho_E to LDS; rows past the list store zeros
//   2. forward      (h1 | hd1) -> A1, the bias in the value half only; z2's epilogue forms h2, hd2, the lane's share of dW3 and
//                   db2, and (zb2 | zdb2) -> A2; h2 is never stored
//   3. dW2          A1 . A2^T over the 64 columns: the value columns give h1 zb2^T, the tangent columns hd1 zdb2^T; both
//                   operands from LDS (the lanes of a half read lines 65 floats apart: no bank conflict), 32 steps a block
//   4. backward     (hb1 | hdb1) = W2 (zb2 | zdb2); the lane that holds both accumulators of a (feature, row) overwrites A1
//                   with (zb1 | zdb1) from its own (h1, hd1); db1
//   5. dW1          X . A1^T over the 64 columns
// Rows of a ragged last tile have G = Gdot = rho_E = 0: then hd1 = hd2 = 0 and zb2 = zb1 = 0, and every term they add is an
// exact zero although the biases make h1 and zdb nonzero there.
//
// Accumulation.  A 32-feature column block of a layer belongs to wave cb (at most eight blocks, eight waves), whatever the
// tile: db1, db2, dW3 stay in that wave's registers for the whole kernel and are summed over the 32 row lanes once at the end;
// db3 and the SSR are per-wave scalars.  dW1 and dW2 (80 blocks of 32 x 32 at the top width) do not fit beside cfw_mm's
// registers: the block owns one partial [1 + P] in the scratch buffer, and after each tile the lane that holds an accumulator
// adds it to its own element -- a plain load, add and store; a store alone on the block's first tile, so nothing is cleared
// beforehand.  Every element has one owner thread: no atomics.  The partials are added by bp.hip's dtrain_reduce_kernel, the
// library's one reduction.  The grid (one block per tile, at most 256) and every order are functions of n_rows and the shapes.
// Built with cfwide.o's flags.
#include "htf_cfwtrain.h"
#include "dtrain_row.h"
#include "pair_mlp.h"

namespace htf {
namespace {

constexpr int kCwtRows = HTF_CFWT_TILE_ROWS;   // rows of a tile: one 32-row half of value, one of tangent
constexpr int kCwtLd = 65;                     // floats between two lines of an image
constexpr int kCwtWaves = 8;
constexpr int kCwtMaxH = HTF_CFW_MAX_H;

__host__ __device__ constexpr int cwt_pad32(int v) { return (v + 31) & ~31; }

struct CwtNet {
    const float *W1, *b1, *W2, *b2, *W3;   // global memory, Keras order
    int D, H1, H2;
};

// cfwide.hip's cfw_mm, statement for statement: acc[hf] += A B over all n_k, A's row i from W, B's column from the image
// line pointer img (at this lane's tile row; half hf -- here the tangent -- is 32 floats on).  TRANS: A[i][k] = W[i][k],
// W [n_i][n_k]; else A[i][k] = W[k][i], W [n_k][n_i].
template <int NH, bool TRANS>
__device__ __forceinline__ void cwt_mm(f32x16 (&acc)[NH], const float *__restrict__ W, int n_i, int n_k, int i, const float *img,
                                       int h) {
    constexpr int NS = TRANS ? 16 : 8;
    const bool row_ok = i < n_i;
    for (int k0 = 0; k0 < n_k; k0 += 2 * NS) {
        float a[NS], b[NH][NS];
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const int k = TRANS ? k0 + NS * h + t : k0 + 2 * t + h;   // (k < the image's lines: a multiple of 32)
            a[t] = 0.f;
            if (row_ok && k < n_k) a[t] = TRANS ? W[(size_t)i * n_k + k] : W[(size_t)k * n_i + i];
#pragma unroll
            for (int hf = 0; hf < NH; ++hf) b[hf][t] = img[k * kCwtLd + 32 * hf];
        }
#pragma unroll
        for (int t = 0; t < NS; ++t) {
#pragma unroll
            for (int hf = 0; hf < NH; ++hf) acc[hf] = HTF_MFMA(a[t], b[hf][t], acc[hf]);
        }
    }
}

// acc = P Q^T contracted over the 64 columns of two image blocks: lane (p, h) supplies P[32 pb + p][k] and Q[32 qb + p][k],
// k = 2 t + h; register v then holds the entry (32 pb + 4 h + f0(v), 32 qb + p).
__device__ __forceinline__ f32x16 cwt_outer(const float *P, const float *Q, int pb, int qb, int p, int h) {
    const float *pa = P + (32 * pb + p) * kCwtLd + h, *qa = Q + (32 * qb + p) * kCwtLd + h;
    f32x16 acc = zero16();
#pragma unroll
    for (int t0 = 0; t0 < 32; t0 += 16) {
        float a[16], b[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            a[t] = pa[2 * (t0 + t)];
            b[t] = qa[2 * (t0 + t)];
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) acc = HTF_MFMA(a[t], b[t], acc);
    }
    return acc;
}

// the block's partial of a matrix [n_p][n_q] takes the tile's 32 x 32 block: each lane its own 16 elements (32 lanes of a half:
// 32 consecutive floats).  first: the block's first tile stores, every later one adds.
__device__ __forceinline__ void cwt_flush(float *out, const f32x16 &acc, int pb, int qb, int n_p, int n_q, int p, int h, bool first) {
    const int j = 32 * qb + p;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int i = 32 * pb + 4 * h + f0(v);
        if (i < n_p && j < n_q) {
            float *q = out + (size_t)i * n_q + j;
            *q = first ? acc[v] : *q + acc[v];
        }
    }
}

template <bool TANH, bool CUT, bool LIST, typename IT>
__global__ __launch_bounds__(64 * kCwtWaves) void wtrain_tile_kernel(const typename Vec4<IT>::type *__restrict__ nlist,
                                                                     const int *__restrict__ index, const int *__restrict__ rows,
                                                                     unsigned n, unsigned B, unsigned NN,
                                                                     const float *__restrict__ weights, const float *__restrict__ mu,
                                                                     int K, int T, int H1, int H2, float gap, float rc,
                                                                     const float4 *__restrict__ rho, float *partials) {
    extern __shared__ float s_mem[];
    const int D = K * T;
    const int D32 = cwt_pad32(D), H1p = cwt_pad32(H1), H2p = cwt_pad32(H2);
    const int nd = D32 / 32, n1 = H1p / 32, n2 = H2p / 32;
    float *X = s_mem, *A1 = X + D32 * kCwtLd, *A2 = A1 + H1p * kCwtLd;
    float *s_mu = A2 + H2p * kCwtLd;
    float *s_re = s_mu + ((K + 3) & ~3);   // [32]: the tile's rho_E, 0 beyond the list
    float *s_red = s_re + kCwtRows;        // [2][8]: the waves' db3 and SSR
    CwtNet net;
    net.W1 = weights; net.b1 = net.W1 + D * H1; net.W2 = net.b1 + H1; net.b2 = net.W2 + H1 * H2; net.W3 = net.b2 + H2;
    net.D = D; net.H1 = H1; net.H2 = H2;
    const int P = (int)dtrain_params((unsigned)D, (unsigned)H1, (unsigned)H2);
    const int oW1 = 1, ob1 = oW1 + D * H1, oW2 = ob1 + H1, ob2 = oW2 + H1 * H2, oW3 = ob2 + H2, ob3 = oW3 + H2;
    float *out = partials + (size_t)blockIdx.x * (1 + P);
    for (int i = threadIdx.x; i < K; i += blockDim.x) s_mu[i] = mu[i];
    __syncthreads();

    const float c_exp = -1.4426950408889634f / gap; // exp(-d^2 / gap) = exp2(c_exp d^2)
    const float c_der = -2.0f / gap;                // d e / d r = c_der (r - mu) e
    const float c_fc = CUT ? cutoff_slope(rc) : 0.f;
    const unsigned lane = threadIdx.x & 63u;
    const int wave = (int)(threadIdx.x >> 6);
    const int p = (int)(lane & 31u), h = (int)(lane >> 5);
    const unsigned ns = (NN + 63u) >> 6;            // slots per lane in use (wave-uniform)
    const unsigned n_tiles = (n + kCwtRows - 1) / kCwtRows;
    const int ia = 32 * wave + p;                   // the row of A this lane supplies in its column block
    const int f_base = 32 * wave + 4 * h;           // accumulator register v: feature f_base + f0(v)

    // column block `wave` of each layer: the bias-like sums of feature f_base + f0(v) over this lane's tile row, all tiles
    float ab1[16], ab2[16], aW3[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) ab1[v] = ab2[v] = aW3[v] = 0.f;
    float ab3 = 0.f, assr = 0.f;

    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const bool first = tile == blockIdx.x;
        // 1. the tile's (G | Gdot): one row per wave at a time, dtrain_rows' steps 0 to 2 with TOTAL
        for (int tr = wave; tr < kCwtRows; tr += kCwtWaves) {
            const unsigned q = tile * kCwtRows + (unsigned)tr;
            float g_mine = 0.f, gd_mine = 0.f, re = 0.f;
            if (q < n) {   // wave-uniform
                unsigned row = q;
                if constexpr (LIST) row = (unsigned)rows[q];
                // 0. the residual (the same value in every lane)
                const float4 pr = rho[row];
                const float rx = pr.x, ry = pr.y, rz = pr.z;
                re = pr.w;
                assr += (rx * rx + ry * ry) + (rz * rz + re * re);
                ab3 += re;

                // 1. this lane's slots: distance, type (-1: contributes nothing), a = ((rho - rho_j) . t) / r
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
                                const float4 rj = rho[j];
                                ax -= rj.x; ay -= rj.y; az -= rj.z;
                            }
                            a[t] = (ax * s.tx + ay * s.tyy + az * s.tz) / s.rr;
                            if constexpr (CUT) cutoff_terms(s.rr, rc, c_fc, fc[t], dfc[t]);
                        }
                    }
                }

                // 2. G and Gdot from the same exponentials: lane t*K + k ends up holding channel k of type t
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
                        float ps = 0.f, pd = 0.f;
#pragma unroll
                        for (int t = 0; t < kDescSlots; ++t)
                            if ((unsigned)t < ns) {
                                ps += ty[t] == tt ? e[t] : 0.f;
                                pd += ty[t] == tt ? ed[t] : 0.f;
                            }
                        const float g = group_sum<64>(ps), gd = group_sum<64>(pd);
                        if ((int)lane == tt * K + k) {
                            g_mine = g;
                            gd_mine = gd;
                        }
                    }
                }
            }
            if ((int)lane < D32) {   // (lanes in [D, D32) and rows beyond the list: explicit zeros)
                X[lane * kCwtLd + tr] = g_mine;
                X[lane * kCwtLd + 32 + tr] = gd_mine;
            }
            if (lane == 0) s_re[tr] = re;
        }
        __syncthreads();

        // 2. forward: (h1 | hd1) -> A1
        if (wave < n1) {
            f32x16 acc[2];
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int f = f_base + f0(v);
                acc[0][v] = f < H1 ? net.b1[f] : 0.f;
                acc[1][v] = 0.f;
            }
            cwt_mm<2, false>(acc, net.W1, H1, D, ia, X + p, h);
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                float *q = A1 + (f_base + f0(v)) * kCwtLd + p;
                const float h1 = desc_act<TANH>(acc[0][v]);
                q[0] = h1;
                q[32] = TANH ? (1.0f - h1 * h1) * acc[1][v] : acc[1][v];
            }
        }
        __syncthreads();
        //    z2's epilogue: dW3, db2 and (zb2 | zdb2) -> A2
        if (wave < n2) {
            f32x16 acc[2];
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int f = f_base + f0(v);
                acc[0][v] = f < H2 ? net.b2[f] : 0.f;
                acc[1][v] = 0.f;
            }
            cwt_mm<2, false>(acc, net.W2, H2, H1, ia, A1 + p, h);
            const float re = s_re[p];
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int f = f_base + f0(v);
                const float w3 = f < H2 ? net.W3[f] : 0.f;
                const float h2 = desc_act<TANH>(acc[0][v]);
                const float s2 = TANH ? 1.0f - h2 * h2 : 1.0f;
                const float hd2 = s2 * acc[1][v];
                const float zdb2 = w3 * s2;
                const float zb2 = TANH ? fmaf(re, zdb2, (-2.0f * (w3 * h2)) * hd2) : re * zdb2;
                aW3[v] += fmaf(re, h2, hd2);
                ab2[v] += zb2;
                float *q = A2 + f * kCwtLd + p;
                q[0] = zb2;
                q[32] = zdb2;
            }
        }
        __syncthreads();

        // 3. dW2 [H1][H2] += A1 . A2^T (before the backward pass overwrites A1)
        for (int blk = wave; blk < n1 * n2; blk += kCwtWaves) {
            const int pb = blk / n2, qb = blk - pb * n2;
            const f32x16 acc = cwt_outer(A1, A2, pb, qb, p, h);
            cwt_flush(out + oW2, acc, pb, qb, H1, H2, p, h, first);
        }
        __syncthreads();

        // 4. backward, in place: (hb1 | hdb1) = W2 (zb2 | zdb2); A1 <- (zb1 | zdb1)
        if (wave < n1) {
            f32x16 acc[2];
            acc[0] = zero16();
            acc[1] = zero16();
            cwt_mm<2, true>(acc, net.W2, H1, H2, ia, A2 + p, h);
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                float *q = A1 + (f_base + f0(v)) * kCwtLd + p;
                const float h1 = q[0], hd1 = q[32];
                const float hb1 = acc[0][v], hdb1 = acc[1][v];
                const float s1 = TANH ? 1.0f - h1 * h1 : 1.0f;
                const float zb1 = TANH ? fmaf(hb1, s1, (-2.0f * (h1 * hd1)) * hdb1) : hb1;
                ab1[v] += zb1;
                q[0] = zb1;
                q[32] = hdb1 * s1;
            }
        }
        __syncthreads();

        // 5. dW1 [D][H1] += X . A1^T
        for (int blk = wave; blk < nd * n1; blk += kCwtWaves) {
            const int pb = blk / n1, qb = blk - pb * n1;
            const f32x16 acc = cwt_outer(X, A1, pb, qb, p, h);
            cwt_flush(out + oW1, acc, pb, qb, D, H1, p, h, first);
        }
        __syncthreads();   // (the next tile's phase 1 writes X and rho_E)
    }

    // the bias-like sums: over the 32 row lanes of a half, then lane 0 of the half stores its 16 features
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int f = f_base + f0(v);
        const float t1 = group_sum<32>(ab1[v]), t2 = group_sum<32>(ab2[v]), t3 = group_sum<32>(aW3[v]);
        if (p == 0 && f < H1) out[ob1 + f] = t1;
        if (p == 0 && f < H2) {
            out[ob2 + f] = t2;
            out[oW3 + f] = t3;
        }
    }
    if (lane == 0) {
        s_red[wave] = ab3;
        s_red[kCwtWaves + wave] = assr;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t3 = 0.f, ts = 0.f;
        for (int w = 0; w < kCwtWaves; ++w) {   // in wave order
            t3 += s_red[w];
            ts += s_red[kCwtWaves + w];
        }
        out[ob3] = t3;
        out[0] = ts;
    }
}

inline size_t cwt_lds(unsigned K, unsigned T, unsigned H1, unsigned H2) {
    const size_t lines = (size_t)cwt_pad32((int)(K * T)) + cwt_pad32((int)H1) + cwt_pad32((int)H2);
    return (lines * kCwtLd + ((K + 3) & ~3u) + kCwtRows + 2 * kCwtWaves) * sizeof(float);
}

// one block per tile of 32 rows until every compute unit has one
inline unsigned cwt_grid(unsigned n_rows) {
    const unsigned tiles = (n_rows + kCwtRows - 1u) / kCwtRows;
    return tiles < HTF_CFWT_MAX_BLOCKS ? tiles : HTF_CFWT_MAX_BLOCKS;
}

// a launch above 64 KiB of dynamic LDS needs the kernel's limit raised first (cfwide.hip's cfw_raise_lds)
template <typename F>
inline int cwt_raise_lds(F kernel, size_t lds) {
    if (lds > 64u * 1024u)
        HTF_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return HTF_OK;
}

inline bool cwt_shape_ok(unsigned K, unsigned T, unsigned H1, unsigned H2) {
    return K >= 2 && T >= 1 && K <= (unsigned)kDescMaxD && T <= (unsigned)kDescMaxD && K * T <= (unsigned)kDescMaxD && H1 >= 1 &&
           H1 <= (unsigned)kCwtMaxH && H2 >= 1 && H2 <= (unsigned)kCwtMaxH;
}

} // namespace
} // namespace htf

extern "C" size_t htf_cfw_scratch_floats(unsigned n_rows, unsigned K, unsigned n_types, unsigned H1, unsigned H2) {
    using namespace htf;
    if (!cwt_shape_ok(K, n_types, H1, H2)) return 0;
    return (size_t)cwt_grid(n_rows) * (1u + dtrain_params(K * n_types, H1, H2));
}

extern "C" int htf_cfw_loss_grad(const void *d_nlist, int nlist_dtype, const int *d_index, unsigned B, unsigned NN, unsigned K,
                                 unsigned n_types, unsigned H1, unsigned H2, int activation, const float *d_weights, const float *d_mu,
                                 float gap, const float *d_rho, float *d_accum, float *d_scratch, const int *d_rows, unsigned n_rows,
                                 float r_cut, htf_stream stream) {
    using namespace htf;
    // (the residual table stands where the entries of desc_row.h have their output)
    int rc = desc_check(d_nlist, nlist_dtype, B, NN, K, n_types, d_mu, gap, d_rho, HTF_F32);
    if (rc != HTF_OK) return rc;
    HTF_REQUIRE(d_weights, "descriptor network: null weights");
    HTF_REQUIRE(cwt_shape_ok(K, n_types, H1, H2), "descriptor network: hidden widths %u, %u outside [1, %d]", H1, H2, kCwtMaxH);
    HTF_REQUIRE(activation == HTF_ACT_LINEAR || activation == HTF_ACT_TANH, "descriptor network: unknown activation %d", activation);
    HTF_REQUIRE(B == 0 || (d_index && d_accum && d_scratch), "descriptor network: null pointer");
    if ((rc = desc_check_rows(B, n_rows, r_cut)) != HTF_OK) return rc;
    const size_t lds = cwt_lds(K, n_types, H1, H2);
    HTF_REQUIRE(lds <= (size_t)HTF_CFW_MAX_LDS_BYTES,
                "descriptor network: a tile of %u x %u x %u needs %zu bytes of LDS, above the %u bytes of one compute unit",
                K * n_types, H1, H2, lds, HTF_CFW_MAX_LDS_BYTES);
    if (!d_accum) return HTF_OK;   // (B = 0 and nothing to zero-fill: no launch)
    const unsigned n = 1u + dtrain_params(K * n_types, H1, H2);
    const unsigned grid = cwt_grid(n_rows);   // (0 for no rows: the reduction alone then writes zeros)
    const hipStream_t s = (hipStream_t)stream;
    if (grid) {
        dispatch_flags([&](auto TANH, auto CUT, auto LIST, auto F64) {
            using IT = scalar_t<F64>;
            auto kernel = wtrain_tile_kernel<TANH, CUT, LIST, IT>;
            if ((rc = cwt_raise_lds(kernel, lds)) != HTF_OK) return;
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * kCwtWaves), lds, s, (const typename Vec4<IT>::type *)d_nlist, d_index,
                               d_rows, n_rows, B, NN, d_weights, d_mu, (int)K, (int)n_types, (int)H1, (int)H2, gap, r_cut,
                               (const float4 *)d_rho, d_scratch);
        }, activation == HTF_ACT_TANH, r_cut > 0.0f, d_rows != nullptr, nlist_dtype == HTF_F64);
        if (rc != HTF_OK) return rc;
        const int rl = check_launch("wtrain_tile_kernel");
        if (rl != HTF_OK) return rl;
    }
    return dtrain_reduce_launch(d_scratch, grid, n, d_accum, s);
}
