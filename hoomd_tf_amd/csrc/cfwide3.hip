// Pass 1 of the conservative forces for wide networks with three hidden layers (include/htf_cfwide3.h,
// htf.DescriptorMLP(conservative=True, dense="mfma", H3=...)): g_i = dE_i/dG_i and E_i of every listed row of
// D -> H1 -> H2 -> H3 -> 1, the dense stack on v_mfma_f32_32x32x2_f32 in exact fp32, hidden layers up to 256 wide.
//
// cfwide.hip's operand convention, unchanged: every layer is computed transposed, Z^T[feature][row] = W^T X^T, features over the
// accumulator rows and tile rows over the lanes.  Lane (p, h) = (lane & 31, lane >> 5) of a 32 x 32 block supplies A[i = p][k_h]
// (a weight, from global memory, unpadded and untransposed) and B[k_h][j = p] (an image line, from LDS); its accumulator
// register v holds feature 8 (v >> 2) + 4 h + (v & 3) of tile row p.
//   forward   A[i][k] = W[k][i]: k = k0 + 2 t + h, a lane's 32 neighbors read 32 consecutive floats of row k of W;
//   backward  A[i][k] = W[i][k]: k = k0 + 16 h + t, t = 0 .. 15: a lane reads a run of 16 consecutive floats of its own row i.
// The bias is the accumulator's initial value; reads past a width return 0 (the guard is on the load).
//
// What is this file's own is the tile.  A block works on R = 64 or 32 listed rows at a time (grid-stride over the tiles) and
// keeps their activations in LDS as three images, one line of R floats per feature, lines R + 1 floats apart:
//
//   XA [max(D32, H3p)][R + 1]   G, then dz3, then g        A1 [H1p][R + 1]   h1, then dz1        A2 [H2p][R + 1]   h2, then dz2
//
// (D32, H1p, H2p, H3p: the widths rounded up to multiples of 32; the lines beyond a width hold zeros or finite values that meet
// zero weights).  A fourth image for dz3 is not needed: G is last read when h1 is formed (stage 2) and g is first written after
// dz3's last use (stage 5), so dz3 lives in G's lines, as many of them as the wider of the two needs.
//
// Stages of a tile, a block barrier between them:
//   1. descriptor   the waves split the R rows; a row is desc_row.h's steps 1 and 2, so G_i is the row kernel's bits; lane c
//                   stores G_i[c] to XA[c][row]
//   2. h1 = act(W1^T G + b1) -> A1
//   3. h2 = act(W2^T h1 + b2) -> A2 (stored: the reverse pass needs act'(h2))
//   4. z3 = W3^T h2 + b3, and its epilogue goes straight on: h3 = act(z3), the lane's share of E_i = h3 . W4 (16 features) to the
//      partials table, and dz3 = W4 act'(h3) -> XA.  h3 itself is never stored.
//   5. dz2 = (W3 dz3) act'(h2) overwrites A2 in place (a lane reads and writes its own elements only)
//   6. dz1 = (W2 dz2) act'(h1) overwrites A1 in place
//   7. g = W1 dz1 -> XA
//   8. store g [row][D] from XA, consecutive threads consecutive channels of a row; E_i = the partials in fixed order + b4.
//      Rows beyond the end of the list store nothing (their columns of XA are zeros: everything stays finite).
//
// LDS rule (the launcher's, include/htf_cfwide3.h has the same text):
//   bytes(R) = 4 ((R + 1) (max(D32, H3p) + H1p + H2p) + 2 R H3p / 32 + K4 + R),   K4 = K rounded up to a multiple of 4
//   R = 64 while bytes(64) <= 160 KB, else R = 32.
// With K = 16: 25 792 bytes at 16 x 32 x 32 x 32, 101 696 at 16 x 160 x 128 x 96, 137 536 at 16 x 128 x 128 x 256, all at
// R = 64; 64 x 256 x 256 x 256 would need 204 096 there and takes 103 616 at R = 32 (103 808 with K = 64, the largest of all).
// So every width triple in [1, 256]^3 with D <= 64 launches.
//
// A stage's 32-wide column blocks go to the waves.  R = 64: with at least as many waves as twice the blocks an item is one
// (block, row half) pair; otherwise a wave keeps both row halves of its block, two accumulators, and every weight it loads
// feeds two instructions.  R = 32: an item is a block, one accumulator; the weights are streamed once per 32 rows, not 64.
// The weights stay in L2.  No atomics, no scratch.  Built with -ffp-contract=on like cfwide.o.
#include "htf_cfwide3.h"
#include "desc_row.h"
#include "pair_mlp.h"

namespace htf {
namespace {

constexpr int kCfw3MaxH = HTF_CFW3_MAX_H;
constexpr int kCfw3MinWaves = 4, kCfw3MaxWaves = 8;

__host__ __device__ constexpr int cfw3_pad32(int v) { return (v + 31) & ~31; }

struct Cfw3Net {
    const float *W1, *b1, *W2, *b2, *W3, *b3, *W4, *b4;   // global memory, Keras order
    int D, H1, H2, H3;
};

// cfwide.hip's cfw_row_channels, statement for statement (desc_rows' step 2 as committee.hip's cmt_row_channels has it): G from
// the lanes' kept slots.  Lane t*K + k returns channel k of type t, every other lane 0.
template <bool CUT>
__device__ __forceinline__ float cfw3_row_channels(const float (&r)[kDescSlots], const float (&fc)[kDescSlots], const int (&ty)[kDescSlots],
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

// cfwide.hip's cfw_mm with the distance between two image lines a template argument.  acc[hf] += A B over all n_k: A's row i
// (this lane's, i < n_i or zeros) from W, B's column from the image line pointer img (already at this lane's tile row; row half
// hf is 32 floats on).  TRANS: A[i][k] = W[i][k], W [n_i][n_k]; else A[i][k] = W[k][i], W [n_k][n_i].  The loads of a chunk are
// issued before its instructions.  The image has at least n_k rounded up to 32 lines.
template <int LD, int NH, bool TRANS>
__device__ __forceinline__ void cfw3_mm(f32x16 (&acc)[NH], const float *__restrict__ W, int n_i, int n_k, int i, const float *img,
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

// One 32-feature block cb of a stage, for NH row halves from hf0 on; R rows in the tile.  STAGE 0: h1 -> A1.  1: h2 -> A2.
// 2: dz3 -> XA and the energy partials.  3: dz2 -> A2 in place.  4: dz1 -> A1 in place.  5: g -> XA.
template <bool TANH, int STAGE, int NH, int R>
__device__ __forceinline__ void cfw3_block(const Cfw3Net &net, float *XA, float *A1, float *A2, float *s_e, int cb, int hf0,
                                           unsigned lane) {
    constexpr int LD = R + 1;
    const int p = (int)(lane & 31u), h = (int)(lane >> 5);
    const int col = 32 * hf0 + p;       // this lane's tile row in the first of its halves
    const int ia = 32 * cb + p;         // the row of A this lane supplies
    const int f_base = 32 * cb + 4 * h; // accumulator register v: feature f_base + f0(v)
    f32x16 acc[NH];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int f = f_base + f0(v);
        float bias = 0.f;
        if constexpr (STAGE == 0) bias = f < net.H1 ? net.b1[f] : 0.f;
        if constexpr (STAGE == 1) bias = f < net.H2 ? net.b2[f] : 0.f;
        if constexpr (STAGE == 2) bias = f < net.H3 ? net.b3[f] : 0.f;
#pragma unroll
        for (int hf = 0; hf < NH; ++hf) acc[hf][v] = bias;
    }
    if constexpr (STAGE == 0) cfw3_mm<LD, NH, false>(acc, net.W1, net.H1, net.D, ia, XA + col, h);
    if constexpr (STAGE == 1) cfw3_mm<LD, NH, false>(acc, net.W2, net.H2, net.H1, ia, A1 + col, h);
    if constexpr (STAGE == 2) cfw3_mm<LD, NH, false>(acc, net.W3, net.H3, net.H2, ia, A2 + col, h);
    if constexpr (STAGE == 3) cfw3_mm<LD, NH, true>(acc, net.W3, net.H2, net.H3, ia, XA + col, h);
    if constexpr (STAGE == 4) cfw3_mm<LD, NH, true>(acc, net.W2, net.H1, net.H2, ia, A2 + col, h);
    if constexpr (STAGE == 5) cfw3_mm<LD, NH, true>(acc, net.W1, net.D, net.H1, ia, A1 + col, h);

    if constexpr (STAGE == 0 || STAGE == 1) {
        float *dst = STAGE == 0 ? A1 : A2;
#pragma unroll
        for (int hf = 0; hf < NH; ++hf)
#pragma unroll
            for (int v = 0; v < 16; ++v) dst[(f_base + f0(v)) * LD + col + 32 * hf] = desc_act<TANH>(acc[hf][v]);
    } else if constexpr (STAGE == 2) {
        float w4[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) w4[v] = f_base + f0(v) < net.H3 ? net.W4[f_base + f0(v)] : 0.f;
#pragma unroll
        for (int hf = 0; hf < NH; ++hf) {
            float e = 0.f;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const float h3 = desc_act<TANH>(acc[hf][v]);
                e = fmaf(h3, w4[v], e);
                XA[(f_base + f0(v)) * LD + col + 32 * hf] = TANH ? w4[v] * (1.0f - h3 * h3) : w4[v];
            }
            s_e[(2 * cb + h) * R + col + 32 * hf] = e;
        }
    } else if constexpr (STAGE == 3 || STAGE == 4) {
        float *dst = STAGE == 3 ? A2 : A1;
#pragma unroll
        for (int hf = 0; hf < NH; ++hf)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                float *q = dst + (f_base + f0(v)) * LD + col + 32 * hf;
                const float hv = *q;
                *q = TANH ? acc[hf][v] * (1.0f - hv * hv) : acc[hf][v];
            }
    } else {
#pragma unroll
        for (int hf = 0; hf < NH; ++hf)
#pragma unroll
            for (int v = 0; v < 16; ++v) XA[(f_base + f0(v)) * LD + col + 32 * hf] = acc[hf][v];
    }
}

// The ncb column blocks of a stage over the block's waves (wave-uniform branches).
template <bool TANH, int STAGE, int R>
__device__ __forceinline__ void cfw3_stage(const Cfw3Net &net, float *XA, float *A1, float *A2, float *s_e, int ncb, int wave,
                                           int nwaves, unsigned lane) {
    if constexpr (R == 32) {
        for (int cb = wave; cb < ncb; cb += nwaves) cfw3_block<TANH, STAGE, 1, R>(net, XA, A1, A2, s_e, cb, 0, lane);
    } else {
        if (2 * ncb <= nwaves) {
            for (int item = wave; item < 2 * ncb; item += nwaves)
                cfw3_block<TANH, STAGE, 1, R>(net, XA, A1, A2, s_e, item >> 1, item & 1, lane);
        } else {
            for (int cb = wave; cb < ncb; cb += nwaves) cfw3_block<TANH, STAGE, 2, R>(net, XA, A1, A2, s_e, cb, 0, lane);
        }
    }
}

template <bool TANH, bool CUT, typename IT, int R>
__global__ __launch_bounds__(64 * kCfw3MaxWaves) void cfw3_tile_kernel(const typename Vec4<IT>::type *__restrict__ nlist,
                                                                       const int *__restrict__ rows, unsigned n, unsigned NN,
                                                                       const float *__restrict__ weights, const float *__restrict__ mu,
                                                                       int K, int T, int H1, int H2, int H3, float gap, float rc,
                                                                       float *__restrict__ g, float *__restrict__ energy) {
    extern __shared__ float s_mem[];
    constexpr int LD = R + 1;
    const int D = K * T;
    const int D32 = cfw3_pad32(D), H1p = cfw3_pad32(H1), H2p = cfw3_pad32(H2), H3p = cfw3_pad32(H3);
    float *XA = s_mem, *A1 = XA + (D32 > H3p ? D32 : H3p) * LD, *A2 = A1 + H1p * LD;
    float *s_e = A2 + H2p * LD;                      // [2 H3p / 32][R]: the energy's partials per (block, lane half)
    float *s_mu = s_e + (H3p / 32) * 2 * R;
    int *s_row = reinterpret_cast<int *>(s_mu + ((K + 3) & ~3));   // [R]: the tile's rows, -1 beyond the list
    Cfw3Net net;
    net.W1 = weights; net.b1 = net.W1 + D * H1; net.W2 = net.b1 + H1; net.b2 = net.W2 + H1 * H2; net.W3 = net.b2 + H2;
    net.b3 = net.W3 + H2 * H3; net.W4 = net.b3 + H3; net.b4 = net.W4 + H3;
    net.D = D; net.H1 = H1; net.H2 = H2; net.H3 = H3;
    for (int i = threadIdx.x; i < K; i += blockDim.x) s_mu[i] = mu[i];
    __syncthreads();

    const float c_exp = -1.4426950408889634f / gap; // exp(-d^2 / gap) = exp2(c_exp d^2)
    const float c_fc = CUT ? cutoff_slope(rc) : 0.f;
    const unsigned lane = threadIdx.x & 63u;
    const int wave = (int)(threadIdx.x >> 6), nwaves = (int)(blockDim.x >> 6);
    const unsigned ns = (NN + 63u) >> 6;            // slots per lane in use (wave-uniform)
    const unsigned n_tiles = (n + R - 1) / R;

    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        // 1. the tile's descriptors: one row per wave at a time
        for (int tr = wave; tr < R; tr += nwaves) {
            const unsigned q = tile * R + (unsigned)tr;
            float g_mine = 0.f;
            int row = -1;
            if (q < n) {   // wave-uniform
                row = (int)q;
                if (rows) row = rows[q];   // (block-uniform; a run-time test keeps the instantiations at sixteen)
                const typename Vec4<IT>::type *rp = nlist + (size_t)(unsigned)row * NN;
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
                g_mine = cfw3_row_channels<CUT>(r, fc, ty, ns, lane, s_mu, K, T, c_exp);
            }
            if ((int)lane < D32) XA[lane * LD + tr] = g_mine;   // (lanes in [D, D32) and rows beyond the list: zeros)
            if (lane == 0) s_row[tr] = row;
        }
        __syncthreads();

        // 2 to 4. forward
        cfw3_stage<TANH, 0, R>(net, XA, A1, A2, s_e, H1p / 32, wave, nwaves, lane);
        __syncthreads();
        cfw3_stage<TANH, 1, R>(net, XA, A1, A2, s_e, H2p / 32, wave, nwaves, lane);
        __syncthreads();
        cfw3_stage<TANH, 2, R>(net, XA, A1, A2, s_e, H3p / 32, wave, nwaves, lane);
        __syncthreads();

        // 5 to 7. backward, in place
        cfw3_stage<TANH, 3, R>(net, XA, A1, A2, s_e, H2p / 32, wave, nwaves, lane);
        __syncthreads();
        cfw3_stage<TANH, 4, R>(net, XA, A1, A2, s_e, H1p / 32, wave, nwaves, lane);
        __syncthreads();
        cfw3_stage<TANH, 5, R>(net, XA, A1, A2, s_e, D32 / 32, wave, nwaves, lane);
        __syncthreads();

        // 8. g [row][D]: consecutive threads, consecutive channels of a row; E from the partials, blocks and halves in order
        for (int idx = threadIdx.x; idx < R * D; idx += blockDim.x) {
            const int tr = idx / D, c = idx - tr * D;
            const int row = s_row[tr];
            if (row >= 0) g[(size_t)(unsigned)row * D + c] = XA[c * LD + tr];
        }
        if (threadIdx.x < R) {
            const int row = s_row[threadIdx.x];
            if (row >= 0) {
                float e = 0.f;
                for (int part = 0; part < (H3p / 32) * 2; ++part) e += s_e[part * R + threadIdx.x];
                energy[(unsigned)row] = e + net.b4[0];
            }
        }
        __syncthreads();   // (the next tile's stage 1 writes XA and the rows)
    }
}

// bytes(R) of the rule at the top of this file
inline size_t cfw3_lds(unsigned K, unsigned T, unsigned H1, unsigned H2, unsigned H3, unsigned R) {
    const size_t d32 = (size_t)cfw3_pad32((int)(K * T)), h3p = (size_t)cfw3_pad32((int)H3);
    const size_t lines = (d32 > h3p ? d32 : h3p) + cfw3_pad32((int)H1) + cfw3_pad32((int)H2);
    return (lines * (R + 1) + (h3p / 32) * 2 * R + ((K + 3) & ~3u) + R) * sizeof(float);
}

// waves of a block, 4 to 8: per 32-wide column block of the widest layer two at R = 64 (an item is then one block and row
// half), one at R = 32
inline unsigned cfw3_waves(unsigned H1, unsigned H2, unsigned H3, unsigned R) {
    const unsigned hmax = H1 > H2 ? (H1 > H3 ? H1 : H3) : (H2 > H3 ? H2 : H3);
    const unsigned w = (R / 32u) * ((unsigned)cfw3_pad32((int)hmax) / 32u);
    return w < (unsigned)kCfw3MinWaves ? kCfw3MinWaves : (w > (unsigned)kCfw3MaxWaves ? kCfw3MaxWaves : w);
}

// a launch above 64 KiB of dynamic LDS needs the kernel's limit raised first (cfwide.hip's cfw_raise_lds)
template <typename F>
inline int cfw3_raise_lds(F kernel, size_t lds) {
    if (lds > 64u * 1024u)
        HTF_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return HTF_OK;
}

} // namespace
} // namespace htf

extern "C" int htf_cfw3_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types, unsigned H1,
                             unsigned H2, unsigned H3, int activation, const float *d_weights, const float *d_mu, float gap,
                             float *d_g, float *d_energy, const int *d_rows, unsigned n_rows, float r_cut, htf_stream stream) {
    using namespace htf;
    int rc = desc_check(d_nlist, nlist_dtype, B, NN, K, n_types, d_mu, gap, d_g, HTF_F32);
    if (rc != HTF_OK) return rc;
    HTF_REQUIRE(d_weights, "descriptor network: null weights");
    HTF_REQUIRE(H1 >= 1 && H1 <= (unsigned)kCfw3MaxH && H2 >= 1 && H2 <= (unsigned)kCfw3MaxH && H3 >= 1 && H3 <= (unsigned)kCfw3MaxH,
                "descriptor network: hidden widths %u, %u, %u outside [1, %d]", H1, H2, H3, kCfw3MaxH);
    HTF_REQUIRE(activation == HTF_ACT_LINEAR || activation == HTF_ACT_TANH, "descriptor network: unknown activation %d", activation);
    if ((rc = desc_check_rows(B, n_rows, r_cut)) != HTF_OK) return rc;
    HTF_REQUIRE(B == 0 || d_energy, "descriptor network: null pointer");
    const bool big = cfw3_lds(K, n_types, H1, H2, H3, 64) <= (size_t)HTF_CFW3_MAX_LDS_BYTES;   // the rule: 64 rows while they fit
    const unsigned R = big ? 64u : 32u;
    const size_t lds = cfw3_lds(K, n_types, H1, H2, H3, R);
    HTF_REQUIRE(lds <= (size_t)HTF_CFW3_MAX_LDS_BYTES,
                "descriptor network: a tile of %u x %u x %u x %u needs %zu bytes of LDS, above the %u bytes of one compute unit",
                K * n_types, H1, H2, H3, lds, HTF_CFW3_MAX_LDS_BYTES);
    if (n_rows == 0) return HTF_OK;
    const unsigned tiles = (n_rows + R - 1) / R;
    const unsigned grid = tiles < kDescMaxBlocks ? tiles : kDescMaxBlocks;
    const unsigned threads = 64u * cfw3_waves(H1, H2, H3, R);
    const hipStream_t s = (hipStream_t)stream;
    dispatch_flags([&](auto TANH, auto CUT, auto F64, auto BIG) {
        using IT = scalar_t<F64>;
        auto kernel = cfw3_tile_kernel<TANH, CUT, IT, BIG ? 64 : 32>;
        if ((rc = cfw3_raise_lds(kernel, lds)) != HTF_OK) return;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, s, (const typename Vec4<IT>::type *)d_nlist, d_rows, n_rows, NN,
                           d_weights, d_mu, (int)K, (int)n_types, (int)H1, (int)H2, (int)H3, gap, r_cut, d_g, d_energy);
    }, activation == HTF_ACT_TANH, r_cut > 0.0f, nlist_dtype == HTF_F64, big);
    if (rc != HTF_OK) return rc;
    return check_launch("cfw3_tile_kernel");
}
