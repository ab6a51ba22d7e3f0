// Force matching on the conservative forces for networks with three hidden layers (include/htf_cfw3train.h,
// htf.DescriptorMLP.deep_loss_gradient, trainable="deep"): cfwtrain.hip's sweep one layer deeper, D -> H1 -> H2 -> H3 -> 1, the
// dense stack on v_mfma_f32_32x32x2_f32 in exact fp32, hidden layers up to 256 wide.
//
// The mathematics is dtrain_row.h's: a row's forward pass carries (value, tangent) along Gdot, a = ((rho_i - rho_j) . t) / r,
// and one reverse pass runs over Q = Edot + rho_E E.  With hd = s zd and s = act'(z) = 1 - h^2 (tanh; 1 for linear, whose
// second-derivative terms vanish), the adjoints (hb, hdb) = (dQ/dh, dQ/dhd) of a layer give
//   zb = hb s - 2 h hd hdb,   zdb = hdb s;      dW = h_below zb^T + hd_below zdb^T,   db = zb,   (hb, hdb)_below = W (zb, zdb),
// started at the top by (hb3, hdb3) = (rho_E w4, w4), dW4 = rho_E h3 + hd3, db4 = rho_E.  cfwtrain.hip's recurrences with one
// more turn.
//
// What is this file's own is the tile.  One block of eight waves works on R = 32 or 16 listed rows at a time (grid-stride over
// the tiles) and keeps FOUR LDS images, one line of 2 R floats per feature, lines LD = 2 R + 1 floats apart -- columns
// 0 .. R - 1 of a line the VALUE of the R rows, columns R .. 2 R - 1 the TANGENT:
//
//   X  [D32][LD]  (G | Gdot)                                   A1 [H1p][LD]  (h1 | hd1), later (zb1 | zdb1)
//   A2 [H2p][LD]  (h2 | hd2), later (zb2 | zdb2)               A3 [H3p][LD]  (zb3 | zdb3)
//
// h2 is stored this time (the reverse pass needs h2 and hd2), and X keeps its lines to the end (dW1 reads it last), so
// cfwide3.hip's shared image does not carry over.  R = 32: a lane (p, h) holds the value and the tangent accumulator of a
// (feature, row) and every weight read feeds two instructions, as in cfwtrain.hip.  R = 16: the 32 columns of a line are the
// 32 columns of ONE instruction -- lane p < 16 works on the value of row p, lane p + 16 on its tangent -- so a weight read still
// carries both; the epilogues, which need value and tangent of an element together, fetch the partner's register (lane ^ 16),
// both lanes form the same result and each stores its own column; only the value lanes add into dW4.
//
// LDS rule (the launcher's, include/htf_cfw3train.h has the same text):
//   bytes(R) = 4 ((2 R + 1) (D32 + H1p + H2p + H3p) + K4 + R + 16),   K4 = K rounded up to a multiple of 4
//   R = 32 while bytes(32) <= 160 KB (at most 608 image lines), else R = 16.
// With K = 16: 108 416 bytes at 16 x 128^3 and 116 736 at 64 x 160 x 128 x 96, both at R = 32; 64 x 256^3 would need 216 576
// there and takes 110 016 at R = 16.  Every width triple in [1, 256]^3 with D <= 64 launches.
//
// Phases of a tile, a block barrier between them:
//   1. descriptor   the waves split the rows; a row is dtrain_rows' steps 0 to 2 with TOTAL; rho_E to LDS; rows past the list
//                   store zeros
//   2. forward      (h1 | hd1) -> A1 and (h2 | hd2) -> A2, the bias in the value half only; z3's epilogue forms h3, hd3, the
//                   lane's share of dW4, and (zb3 | zdb3) -> A3; h3 is never stored
//   3. dW3          A2 . A3^T over the 2 R columns: the value columns give h2 zb3^T, the tangent columns hd2 zdb3^T
//   4. backward     (hb2 | hdb2) = W3 (zb3 | zdb3); A2 <- (zb2 | zdb2) from its own (h2, hd2)
//   5. dW2          A1 . A2^T
//   6. backward     (hb1 | hdb1) = W2 (zb2 | zdb2); A1 <- (zb1 | zdb1)
//   7. dW1          X . A1^T; db1, db2, db3 from the images
// Rows of a ragged last tile have G = Gdot = rho_E = 0: then every hd and every zb is 0, and each term they add is an exact
// zero although the biases make h and zdb nonzero there.
//
// Accumulation.  The 32-feature column block cb of every layer belongs to wave cb, whatever the tile: dW4 stays in that wave's
// registers for the whole kernel and is summed over the row lanes once at the end.  db1, db2, db3 are the row sums of zb1, zb2,
// zb3, which the value halves of A1, A2, A3 all hold once phase 6 is done: in phase 7 thread 2 f + c adds half c of line f of
// each image into three registers of its own (cfwtrain.hip's sixteen registers per layer and lane, 64 with a third layer
// and dW4, spilled in the 32-row forms).  db4 and the SSR are per-wave scalars.  dW1, dW2 and dW3 go to the block's partial
// [1 + P] in the scratch buffer after each tile, the lane that holds an accumulator adding it to its own element -- a plain
// load, add and store; a store alone on the block's first tile.  Every element has one owner thread: no atomics.  The
// partials are added by bp.hip's dtrain_reduce_kernel.  The grid (one block per tile, at most 256) and every order are
// functions of n_rows and the shapes.  Built with cfwide.o's flags.
#include "htf_cfw3train.h"
#include "dtrain_row.h"
#include "pair_mlp.h"

namespace htf {
namespace {

constexpr int kC3tWaves = 8;
constexpr int kC3tMaxH = HTF_CFW3_MAX_H;

__host__ __device__ constexpr int c3t_pad32(int v) { return (v + 31) & ~31; }

__host__ __device__ inline unsigned c3t_params(unsigned D, unsigned H1, unsigned H2, unsigned H3) {
    return D * H1 + H1 + H1 * H2 + H2 + H2 * H3 + H3 + H3 + 1;
}

// cfwide3.hip's cfw3_mm, statement for statement: acc[hf] += A B over all n_k, A's row i from W, B's column from the image
// line pointer img (at this lane's column; half hf is 32 floats on).  TRANS: A[i][k] = W[i][k], W [n_i][n_k]; else
// A[i][k] = W[k][i], W [n_k][n_i].  The image has at least n_k rounded up to 32 lines.
template <int LD, int NH, bool TRANS>
__device__ __forceinline__ void c3t_mm(f32x16 (&acc)[NH], const float *__restrict__ W, int n_i, int n_k, int i, const float *img,
                                       int h) {
    constexpr int NS = TRANS ? 16 : 8;
    const bool row_ok = i < n_i;
    for (int k0 = 0; k0 < n_k; k0 += 2 * NS) {
        float a[NS], b[NH][NS];
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const int k = TRANS ? k0 + NS * h + t : k0 + 2 * t + h;
            a[t] = 0.f;
            if (row_ok && k < n_k) a[t] = TRANS ? W[(size_t)i * n_k + k] : W[(size_t)k * n_i + i];
#pragma unroll
            for (int hf = 0; hf < NH; ++hf) b[hf][t] = img[k * LD + 32 * hf];
        }
#pragma unroll
        for (int t = 0; t < NS; ++t) {
#pragma unroll
            for (int hf = 0; hf < NH; ++hf) acc[hf] = HTF_MFMA(a[t], b[hf][t], acc[hf]);
        }
    }
}

// What a lane sees of a tile of R rows: its row r, whether it is a value lane (lo; every lane at R = 32), and how value and
// tangent of an element reach it and leave it.
template <int R>
struct C3tLane {
    static constexpr int LD = 2 * R + 1, NH = R / 16;
    int p, r;
    bool lo;

    __device__ __forceinline__ explicit C3tLane(int p_) : p(p_), r(p_ & (R - 1)), lo(p_ < R) {}

    // the accumulators' initial value: the bias in the value columns, zero in the tangent's
    __device__ __forceinline__ void init(f32x16 (&acc)[NH], int v, float bias) const {
        if constexpr (R == 32) {
            acc[0][v] = bias;
            acc[1][v] = 0.f;
        } else {
            acc[0][v] = lo ? bias : 0.f;
        }
    }

    // (value, tangent) of register v at row r
    __device__ __forceinline__ void pair(const f32x16 (&acc)[NH], int v, float &val, float &tan) const {
        if constexpr (R == 32) {
            val = acc[0][v];
            tan = acc[1][v];
        } else {
            const float own = acc[0][v], other = __shfl_xor(own, 16);
            val = lo ? own : other;
            tan = lo ? other : own;
        }
    }

    // (value, tangent) of row r to an image line: both at R = 32, this lane's own column at R = 16
    __device__ __forceinline__ void store(float *line, float val, float tan) const {
        if constexpr (R == 32) {
            line[r] = val;
            line[R + r] = tan;
        } else {
            line[p] = lo ? val : tan;
        }
    }
};

// acc = P Q^T contracted over the 2 R columns of two image blocks: lane (p, h) supplies P[32 pb + p][k] and Q[32 qb + p][k],
// k = 2 t + h; register v then holds the entry (32 pb + 4 h + f0(v), 32 qb + p).
template <int R>
__device__ __forceinline__ f32x16 c3t_outer(const float *P, const float *Q, int pb, int qb, int p, int h) {
    constexpr int LD = 2 * R + 1;
    const float *pa = P + (32 * pb + p) * LD + h, *qa = Q + (32 * qb + p) * LD + h;
    f32x16 acc = zero16();
#pragma unroll
    for (int t0 = 0; t0 < R; t0 += 16) {
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
__device__ __forceinline__ void c3t_flush(float *out, const f32x16 &acc, int pb, int qb, int n_p, int n_q, int p, int h, bool first) {
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

// dW [n_p][n_q] += P . Q^T, the 32 x 32 blocks over the waves
template <int R>
__device__ __forceinline__ void c3t_dw(float *out, const float *P, const float *Q, int n_p, int n_q, int wave, int p, int h, bool first) {
    const int npb = c3t_pad32(n_p) / 32, nqb = c3t_pad32(n_q) / 32;
    for (int blk = wave; blk < npb * nqb; blk += kC3tWaves) {
        const int pb = blk / nqb, qb = blk - pb * nqb;
        const f32x16 acc = c3t_outer<R>(P, Q, pb, qb, p, h);
        c3t_flush(out, acc, pb, qb, n_p, n_q, p, h, first);
    }
}

// forward of a hidden layer that is stored: (h | hd) = act(W^T (below) + b) with its tangent -> image `dst`, column block `wave`
template <bool TANH, int R>
__device__ __forceinline__ void c3t_forward(const C3tLane<R> &ln, const float *__restrict__ W, const float *__restrict__ bias, int n_out,
                                            int n_in, const float *below, float *dst, int wave, int h) {
    constexpr int LD = C3tLane<R>::LD, NH = C3tLane<R>::NH;
    const int f_base = 32 * wave + 4 * h;
    f32x16 acc[NH];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int f = f_base + f0(v);
        ln.init(acc, v, f < n_out ? bias[f] : 0.f);
    }
    c3t_mm<LD, NH, false>(acc, W, n_out, n_in, 32 * wave + (ln.p & 31), below + ln.p, h);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        float z, zd;
        ln.pair(acc, v, z, zd);
        const float hv = desc_act<TANH>(z);
        ln.store(dst + (f_base + f0(v)) * LD, hv, TANH ? (1.0f - hv * hv) * zd : zd);
    }
}

// reverse through a stored hidden layer, in place: (hb | hdb) = W (zb | zdb)_above; img <- (zb | zdb) from its own (h, hd)
template <bool TANH, int R>
__device__ __forceinline__ void c3t_backward(const C3tLane<R> &ln, const float *__restrict__ W, int n_here, int n_above, const float *above,
                                             float *img, int wave, int h) {
    constexpr int LD = C3tLane<R>::LD, NH = C3tLane<R>::NH;
    const int f_base = 32 * wave + 4 * h;
    f32x16 acc[NH];
#pragma unroll
    for (int hf = 0; hf < NH; ++hf) acc[hf] = zero16();
    c3t_mm<LD, NH, true>(acc, W, n_here, n_above, 32 * wave + (ln.p & 31), above + ln.p, h);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        float *line = img + (f_base + f0(v)) * LD;
        const float hv = line[ln.r], hd = line[R + ln.r];
        float hb, hdb;
        ln.pair(acc, v, hb, hdb);
        const float s = TANH ? 1.0f - hv * hv : 1.0f;
        const float zb = TANH ? fmaf(hb, s, (-2.0f * (hv * hd)) * hdb) : hb;
        ln.store(line, zb, hdb * s);
    }
}

template <bool TANH, bool CUT, typename IT, int R>
__global__ __launch_bounds__(64 * kC3tWaves) void c3train_tile_kernel(const typename Vec4<IT>::type *__restrict__ nlist,
                                                                      const int *__restrict__ index, const int *__restrict__ rows,
                                                                      unsigned n, unsigned B, unsigned NN,
                                                                      const float *__restrict__ weights, const float *__restrict__ mu,
                                                                      int K, int T, int H1, int H2, int H3, float gap, float rc,
                                                                      const float4 *__restrict__ rho, float *partials) {
    extern __shared__ float s_mem[];
    constexpr int LD = 2 * R + 1, NH = R / 16;
    const int D = K * T;
    const int D32 = c3t_pad32(D), H1p = c3t_pad32(H1), H2p = c3t_pad32(H2), H3p = c3t_pad32(H3);
    float *X = s_mem, *A1 = X + D32 * LD, *A2 = A1 + H1p * LD, *A3 = A2 + H2p * LD;
    float *s_mu = A3 + H3p * LD;
    float *s_re = s_mu + ((K + 3) & ~3);   // [R]: the tile's rho_E, 0 beyond the list
    float *s_red = s_re + R;               // [2][8]: the waves' db4 and SSR
    const float *W1 = weights, *b1 = W1 + D * H1, *W2 = b1 + H1, *b2 = W2 + H1 * H2, *W3 = b2 + H2, *b3 = W3 + H2 * H3, *W4 = b3 + H3;
    const int oW1 = 1, ob1 = oW1 + D * H1, oW2 = ob1 + H1, ob2 = oW2 + H1 * H2, oW3 = ob2 + H2, ob3 = oW3 + H2 * H3, oW4 = ob3 + H3,
              ob4 = oW4 + H3;
    float *out = partials + (size_t)blockIdx.x * (size_t)(ob4 + 1);   // (ob4 + 1 = 1 + P)
    for (int i = threadIdx.x; i < K; i += blockDim.x) s_mu[i] = mu[i];
    __syncthreads();

    const float c_exp = -1.4426950408889634f / gap; // exp(-d^2 / gap) = exp2(c_exp d^2)
    const float c_der = -2.0f / gap;                // d e / d r = c_der (r - mu) e
    const float c_fc = CUT ? cutoff_slope(rc) : 0.f;
    const unsigned lane = threadIdx.x & 63u;
    const int wave = (int)(threadIdx.x >> 6);
    const int p = (int)(lane & 31u), h = (int)(lane >> 5);
    const C3tLane<R> ln(p);
    const unsigned ns = (NN + 63u) >> 6;            // slots per lane in use (wave-uniform)
    const unsigned n_tiles = (n + R - 1) / R;
    const int f_base = 32 * wave + 4 * h;           // accumulator register v: feature f_base + f0(v)

    // column block `wave` of the last layer: dW4 of feature f_base + f0(v) over this lane's tile row, all tiles
    float aW4[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) aW4[v] = 0.f;
    // db1, db2, db3 of feature bf over the columns [bc, bc + R / 2) of every tile: two threads a feature
    const int bf = (int)(threadIdx.x >> 1), bc = (int)(threadIdx.x & 1u) * (R / 2);
    float ab1 = 0.f, ab2 = 0.f, ab3 = 0.f;
    float ab4 = 0.f, assr = 0.f;

    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const bool first = tile == blockIdx.x;
        // 1. the tile's (G | Gdot): one row per wave at a time, dtrain_rows' steps 0 to 2 with TOTAL (cfwtrain.hip's statements)
        for (int tr = wave; tr < R; tr += kC3tWaves) {
            const unsigned q = tile * R + (unsigned)tr;
            float g_mine = 0.f, gd_mine = 0.f, re = 0.f;
            if (q < n) {   // wave-uniform
                unsigned row = q;
                if (rows) row = (unsigned)rows[q];   // (block-uniform; a run-time test keeps the instantiations at sixteen)
                // 0. the residual (the same value in every lane)
                const float4 pr = rho[row];
                const float rx = pr.x, ry = pr.y, rz = pr.z;
                re = pr.w;
                assr += (rx * rx + ry * ry) + (rz * rz + re * re);
                ab4 += re;

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
                X[lane * LD + tr] = g_mine;
                X[lane * LD + R + tr] = gd_mine;
            }
            if (lane == 0) s_re[tr] = re;
        }
        __syncthreads();

        // 2. forward: (h1 | hd1) -> A1, (h2 | hd2) -> A2
        if (wave < H1p / 32) c3t_forward<TANH, R>(ln, W1, b1, H1, D, X, A1, wave, h);
        __syncthreads();
        if (wave < H2p / 32) c3t_forward<TANH, R>(ln, W2, b2, H2, H1, A1, A2, wave, h);
        __syncthreads();
        //    z3's epilogue: dW4 and (zb3 | zdb3) -> A3
        if (wave < H3p / 32) {
            f32x16 acc[NH];
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int f = f_base + f0(v);
                ln.init(acc, v, f < H3 ? b3[f] : 0.f);
            }
            c3t_mm<LD, NH, false>(acc, W3, H3, H2, 32 * wave + p, A2 + p, h);
            const float re = s_re[ln.r];
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int f = f_base + f0(v);
                const float w4 = f < H3 ? W4[f] : 0.f;
                float z, zd;
                ln.pair(acc, v, z, zd);
                const float h3 = desc_act<TANH>(z);
                const float s3 = TANH ? 1.0f - h3 * h3 : 1.0f;
                const float hd3 = s3 * zd;
                const float zdb3 = w4 * s3;
                const float zb3 = TANH ? fmaf(re, zdb3, (-2.0f * (w4 * h3)) * hd3) : re * zdb3;
                if (ln.lo) aW4[v] += fmaf(re, h3, hd3);
                ln.store(A3 + f * LD, zb3, zdb3);
            }
        }
        __syncthreads();

        // 3. dW3 [H2][H3] += A2 . A3^T (before the backward pass overwrites A2)
        c3t_dw<R>(out + oW3, A2, A3, H2, H3, wave, p, h, first);
        __syncthreads();
        // 4. backward, in place: A2 <- (zb2 | zdb2)
        if (wave < H2p / 32) c3t_backward<TANH, R>(ln, W3, H2, H3, A3, A2, wave, h);
        __syncthreads();
        // 5. dW2 [H1][H2] += A1 . A2^T
        c3t_dw<R>(out + oW2, A1, A2, H1, H2, wave, p, h, first);
        __syncthreads();
        // 6. backward, in place: A1 <- (zb1 | zdb1)
        if (wave < H1p / 32) c3t_backward<TANH, R>(ln, W2, H1, H2, A2, A1, wave, h);
        __syncthreads();
        // 7. dW1 [D][H1] += X . A1^T
        c3t_dw<R>(out + oW1, X, A1, D, H1, wave, p, h, first);
        //    db1, db2, db3: the value halves of the three images now hold zb1, zb2, zb3 (padding lines: zeros)
#pragma unroll
        for (int c = 0; c < R / 2; ++c) {
            if (bf < H1p) ab1 += A1[bf * LD + bc + c];
            if (bf < H2p) ab2 += A2[bf * LD + bc + c];
            if (bf < H3p) ab3 += A3[bf * LD + bc + c];
        }
        __syncthreads();   // (the next tile's phase 1 writes X and rho_E)
    }

    // dW4: over the 32 lanes of a half (the tangent lanes of a 16-row tile hold zeros), then lane 0 of the half stores its 16
    // features; the biases: a feature's two column halves, the even thread stores
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int f = f_base + f0(v);
        const float t4 = group_sum<32>(aW4[v]);
        if (p == 0 && f < H3 && wave < H3p / 32) out[oW4 + f] = t4;
    }
    {
        const float t1 = group_sum<2>(ab1), t2 = group_sum<2>(ab2), t3 = group_sum<2>(ab3);
        if (bc == 0 && bf < H1) out[ob1 + bf] = t1;
        if (bc == 0 && bf < H2) out[ob2 + bf] = t2;
        if (bc == 0 && bf < H3) out[ob3 + bf] = t3;
    }
    if (lane == 0) {
        s_red[wave] = ab4;
        s_red[kC3tWaves + wave] = assr;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t4 = 0.f, ts = 0.f;
        for (int w = 0; w < kC3tWaves; ++w) {   // in wave order
            t4 += s_red[w];
            ts += s_red[kC3tWaves + w];
        }
        out[ob4] = t4;
        out[0] = ts;
    }
}

// bytes(R) of the rule at the top of this file
inline size_t c3t_lds(unsigned K, unsigned T, unsigned H1, unsigned H2, unsigned H3, unsigned R) {
    const size_t lines = (size_t)c3t_pad32((int)(K * T)) + c3t_pad32((int)H1) + c3t_pad32((int)H2) + c3t_pad32((int)H3);
    return (lines * (2 * R + 1) + ((K + 3) & ~3u) + R + 2 * kC3tWaves) * sizeof(float);
}

inline bool c3t_shape_ok(unsigned K, unsigned T, unsigned H1, unsigned H2, unsigned H3) {
    const unsigned hmax = (unsigned)kC3tMaxH;
    return K >= 2 && T >= 1 && K <= (unsigned)kDescMaxD && T <= (unsigned)kDescMaxD && K * T <= (unsigned)kDescMaxD && H1 >= 1 &&
           H1 <= hmax && H2 >= 1 && H2 <= hmax && H3 >= 1 && H3 <= hmax;
}

// the rule: 32 rows while their images fit, else 16
inline unsigned c3t_tile_rows(unsigned K, unsigned T, unsigned H1, unsigned H2, unsigned H3) {
    return c3t_lds(K, T, H1, H2, H3, 32) <= (size_t)HTF_CFW3_MAX_LDS_BYTES ? 32u : 16u;
}

// one block per tile until every compute unit has one
inline unsigned c3t_grid(unsigned n_rows, unsigned R) {
    const unsigned tiles = (n_rows + R - 1u) / R;
    return tiles < HTF_CFW3T_MAX_BLOCKS ? tiles : HTF_CFW3T_MAX_BLOCKS;
}

// a launch above 64 KiB of dynamic LDS needs the kernel's limit raised first (cfwide.hip's cfw_raise_lds)
template <typename F>
inline int c3t_raise_lds(F kernel, size_t lds) {
    if (lds > 64u * 1024u)
        HTF_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return HTF_OK;
}

} // namespace
} // namespace htf

extern "C" size_t htf_cfw3_scratch_floats(unsigned n_rows, unsigned K, unsigned n_types, unsigned H1, unsigned H2, unsigned H3) {
    using namespace htf;
    if (!c3t_shape_ok(K, n_types, H1, H2, H3)) return 0;
    return (size_t)c3t_grid(n_rows, c3t_tile_rows(K, n_types, H1, H2, H3)) * (1u + c3t_params(K * n_types, H1, H2, H3));
}

extern "C" int htf_cfw3_loss_grad(const void *d_nlist, int nlist_dtype, const int *d_index, unsigned B, unsigned NN, unsigned K,
                                  unsigned n_types, unsigned H1, unsigned H2, unsigned H3, int activation, const float *d_weights,
                                  const float *d_mu, float gap, const float *d_rho, float *d_accum, float *d_scratch,
                                  const int *d_rows, unsigned n_rows, float r_cut, htf_stream stream) {
    using namespace htf;
    // (the residual table stands where the entries of desc_row.h have their output)
    int rc = desc_check(d_nlist, nlist_dtype, B, NN, K, n_types, d_mu, gap, d_rho, HTF_F32);
    if (rc != HTF_OK) return rc;
    HTF_REQUIRE(d_weights, "descriptor network: null weights");
    HTF_REQUIRE(c3t_shape_ok(K, n_types, H1, H2, H3), "descriptor network: hidden widths %u, %u, %u outside [1, %d]", H1, H2, H3,
                kC3tMaxH);
    HTF_REQUIRE(activation == HTF_ACT_LINEAR || activation == HTF_ACT_TANH, "descriptor network: unknown activation %d", activation);
    HTF_REQUIRE(B == 0 || (d_index && d_accum && d_scratch), "descriptor network: null pointer");
    if ((rc = desc_check_rows(B, n_rows, r_cut)) != HTF_OK) return rc;
    const unsigned R = c3t_tile_rows(K, n_types, H1, H2, H3);
    const size_t lds = c3t_lds(K, n_types, H1, H2, H3, R);
    HTF_REQUIRE(lds <= (size_t)HTF_CFW3_MAX_LDS_BYTES,
                "descriptor network: a tile of %u x %u x %u x %u needs %zu bytes of LDS, above the %u bytes of one compute unit",
                K * n_types, H1, H2, H3, lds, HTF_CFW3_MAX_LDS_BYTES);
    if (!d_accum) return HTF_OK;   // (B = 0 and nothing to zero-fill: no launch)
    const unsigned n = 1u + c3t_params(K * n_types, H1, H2, H3);
    const unsigned grid = c3t_grid(n_rows, R);   // (0 for no rows: the reduction alone then writes zeros)
    const hipStream_t s = (hipStream_t)stream;
    if (grid) {
        dispatch_flags([&](auto TANH, auto CUT, auto F64, auto SMALL) {
            using IT = scalar_t<F64>;
            auto kernel = c3train_tile_kernel<TANH, CUT, IT, SMALL ? 16 : 32>;
            if ((rc = c3t_raise_lds(kernel, lds)) != HTF_OK) return;
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * kC3tWaves), lds, s, (const typename Vec4<IT>::type *)d_nlist, d_index,
                               d_rows, n_rows, B, NN, d_weights, d_mu, (int)K, (int)n_types, (int)H1, (int)H2, (int)H3, gap, r_cut,
                               (const float4 *)d_rho, d_scratch);
        }, activation == HTF_ACT_TANH, r_cut > 0.0f, nlist_dtype == HTF_F64, R == 16u);
        if (rc != HTF_OK) return rc;
        const int rl = check_launch("c3train_tile_kernel");
        if (rl != HTF_OK) return rl;
    }
    return dtrain_reduce_launch(d_scratch, grid, n, d_accum, s);
}
