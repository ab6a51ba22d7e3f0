// Pass 1 of the conservative forces for wide networks (include/htf_cfwide.h, htf.DescriptorMLP(conservative=True, dense="mfma")):
// g_i = dE_i/dG_i and E_i of every listed row, the dense stack on v_mfma_f32_32x32x2_f32, hidden layers up to 256 wide.
//
// One block works on a tile of 64 listed rows at a time (grid-stride over the tiles) and keeps the tile's activations in LDS as
// three images, one line of 64 floats per feature, lines 65 floats apart:
//
//   X  [D32 ][65]   G, later g        A1 [H1p][65]   h1, later dz1        A2 [H2p][65]   dz2
//
// (D32, H1p, H2p: the widths rounded up to multiples of 32; the lines beyond a width hold zeros).  Every layer is computed
// transposed, Z^T[feature][row] = W^T X^T, pair_mlp.hip's convention: features run over the accumulator rows, tile rows over the
// lanes.  Lane (p, h) = (lane & 31, lane >> 5) of a 32 x 32 block supplies A[i = p][k_h] (a weight, from global memory) and
// B[k_h][j = p] (an image line, from LDS), and its accumulator register v holds feature 8 (v >> 2) + 4 h + (v & 3) of tile row
// p: written to the next image at [feature][row], the 32 lanes of a half store to 32 consecutive floats.  Which contraction
// index the two halves take in a step is free as long as A and B agree, and that is what keeps the weights unpadded and
// untransposed in global memory:
//   forward   A[i][k] = W[k][i]: k = k0 + 2 t + h, a lane's 32 neighbors read 32 consecutive floats of row k of W;
//   backward  A[i][k] = W[i][k]: k = k0 + 16 h + t, t = 0 .. 15: a lane reads a run of 16 consecutive floats of its own row i
//             of W, the two halves of the wave the two halves of a 128-byte line.  No staging slab, no transposed copy.
// Reads past a width return 0 (the guard is on the load, nothing is padded in global memory).
//
// Phases of a tile, a block barrier between them:
//   1. descriptor   the waves split the 64 rows; a row is desc_row.h's steps 1 and 2 (desc_slot, the keep rule, the cutoff
//                   terms, the fixed-order wave sums), so G_i is the row kernel's bits; lane c stores G_i[c] to X[c][row]
//   2. forward      h1 = act(W1^T G + b1) -> A1 (the bias is the accumulator's initial value); z2 likewise, and its epilogue
//                   goes straight on: h2 = act(z2), the lane's share of E_i = h2 . W3 (16 features) to a partials table, and
//                   dz2 = W3 act'(h2) -> A2.  h2 itself is never stored.
//   3. backward     dz1 = (W2 dz2) act'(h1) overwrites A1 in place (a lane reads and writes its own elements only);
//                   g = W1 dz1 overwrites X
//   4. store        g [row][D] from X, consecutive threads consecutive channels of a row; E_i = the partials in fixed order + b3.
//                   Rows beyond the end of the list store nothing (their columns of X are zeros: everything stays finite).
// A layer's 32-wide column blocks go to the waves.  With at least as many waves as twice the blocks an item is one (block, row
// half) pair; otherwise a wave keeps both row halves of its block, two accumulators, and every weight it loads feeds two
// instructions.  The weights stay in L2 and are streamed once forward and once backward per tile.
//
// The launcher sizes the block (4 to 8 waves) and the LDS from the actual D, H1, H2: 25 KB at 16 x 32 x 32, several blocks per
// compute unit; 151 KB at 64 x 256 x 256, one block.  No atomics, no scratch.  Built with -ffp-contract=on like cforce.o.
#include "htf_cfwide.h"
#include "desc_row.h"
#include "pair_mlp.h"

namespace htf {
namespace {

constexpr int kCfwRows = 64;      // rows of a tile: two 32-row halves
constexpr int kCfwLd = 65;        // floats between two lines of an image (odd: phase 1 and the store walk down a column)
constexpr int kCfwMaxH = HTF_CFW_MAX_H;
constexpr int kCfwMinWaves = 4, kCfwMaxWaves = 8;

__host__ __device__ constexpr int cfw_pad32(int v) { return (v + 31) & ~31; }

struct CfwNet {
    const float *W1, *b1, *W2, *b2, *W3, *b3;   // global memory, Keras order
    int D, H1, H2;
};

// desc_rows' step 2 (desc_row.h) as committee.hip's cmt_row_channels has it, statement for statement: G from the lanes' kept
// slots.  Lane t*K + k returns channel k of type t, every other lane 0.
template <bool CUT>
__device__ __forceinline__ float cfw_row_channels(const float (&r)[kDescSlots], const float (&fc)[kDescSlots], const int (&ty)[kDescSlots],
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

// acc[hf] += A B over all n_k: A's row i (this lane's, i < n_i or zeros) from W, B's column from the image line pointer img
// (already at this lane's tile row; row half hf is 32 floats on).  TRANS: A[i][k] = W[i][k], W [n_i][n_k]; else A[i][k] = W[k][i],
// W [n_k][n_i].  The loads of a chunk are issued before its instructions: 8 or 16 weights and as many image values per half.
template <int NH, bool TRANS>
__device__ __forceinline__ void cfw_mm(f32x16 (&acc)[NH], const float *__restrict__ W, int n_i, int n_k, int i, const float *img,
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
            for (int hf = 0; hf < NH; ++hf) b[hf][t] = img[k * kCfwLd + 32 * hf];
        }
#pragma unroll
        for (int t = 0; t < NS; ++t) {
#pragma unroll
            for (int hf = 0; hf < NH; ++hf) acc[hf] = HTF_MFMA(a[t], b[hf][t], acc[hf]);
        }
    }
}

// One 32-feature block cb of a stage, for NH row halves from hf0 on.  STAGE 0: h1 -> A1.  1: dz2 -> A2 and the energy partials.
// 2: dz1 -> A1 in place.  3: g -> X.
template <bool TANH, int STAGE, int NH>
__device__ __forceinline__ void cfw_block(const CfwNet &net, float *X, float *A1, float *A2, float *s_e, int cb, int hf0,
                                          unsigned lane) {
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
#pragma unroll
        for (int hf = 0; hf < NH; ++hf) acc[hf][v] = bias;
    }
    if constexpr (STAGE == 0) cfw_mm<NH, false>(acc, net.W1, net.H1, net.D, ia, X + col, h);
    if constexpr (STAGE == 1) cfw_mm<NH, false>(acc, net.W2, net.H2, net.H1, ia, A1 + col, h);
    if constexpr (STAGE == 2) cfw_mm<NH, true>(acc, net.W2, net.H1, net.H2, ia, A2 + col, h);
    if constexpr (STAGE == 3) cfw_mm<NH, true>(acc, net.W1, net.D, net.H1, ia, A1 + col, h);

    if constexpr (STAGE == 0) {
#pragma unroll
        for (int hf = 0; hf < NH; ++hf)
#pragma unroll
            for (int v = 0; v < 16; ++v) A1[(f_base + f0(v)) * kCfwLd + col + 32 * hf] = desc_act<TANH>(acc[hf][v]);
    } else if constexpr (STAGE == 1) {
        float w3[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) w3[v] = f_base + f0(v) < net.H2 ? net.W3[f_base + f0(v)] : 0.f;
#pragma unroll
        for (int hf = 0; hf < NH; ++hf) {
            float e = 0.f;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const float h2 = desc_act<TANH>(acc[hf][v]);
                e = fmaf(h2, w3[v], e);
                A2[(f_base + f0(v)) * kCfwLd + col + 32 * hf] = TANH ? w3[v] * (1.0f - h2 * h2) : w3[v];
            }
            s_e[(2 * cb + h) * kCfwRows + col + 32 * hf] = e;
        }
    } else if constexpr (STAGE == 2) {
#pragma unroll
        for (int hf = 0; hf < NH; ++hf)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                float *q = A1 + (f_base + f0(v)) * kCfwLd + col + 32 * hf;
                const float h1 = *q;
                *q = TANH ? acc[hf][v] * (1.0f - h1 * h1) : acc[hf][v];
            }
    } else {
#pragma unroll
        for (int hf = 0; hf < NH; ++hf)
#pragma unroll
            for (int v = 0; v < 16; ++v) X[(f_base + f0(v)) * kCfwLd + col + 32 * hf] = acc[hf][v];
    }
}

// The ncb column blocks of a stage over the block's waves (wave-uniform branches).
template <bool TANH, int STAGE>
__device__ __forceinline__ void cfw_stage(const CfwNet &net, float *X, float *A1, float *A2, float *s_e, int ncb, int wave, int nwaves,
                                          unsigned lane) {
    if (2 * ncb <= nwaves) {
        for (int item = wave; item < 2 * ncb; item += nwaves) cfw_block<TANH, STAGE, 1>(net, X, A1, A2, s_e, item >> 1, item & 1, lane);
    } else {
        for (int cb = wave; cb < ncb; cb += nwaves) cfw_block<TANH, STAGE, 2>(net, X, A1, A2, s_e, cb, 0, lane);
    }
}

template <bool TANH, bool CUT, bool LIST, typename IT>
__global__ __launch_bounds__(64 * kCfwMaxWaves) void cfw_tile_kernel(const typename Vec4<IT>::type *__restrict__ nlist,
                                                                     const int *__restrict__ rows, unsigned n, unsigned NN,
                                                                     const float *__restrict__ weights, const float *__restrict__ mu,
                                                                     int K, int T, int H1, int H2, float gap, float rc,
                                                                     float *__restrict__ g, float *__restrict__ energy) {
    extern __shared__ float s_mem[];
    const int D = K * T;
    const int D32 = cfw_pad32(D), H1p = cfw_pad32(H1), H2p = cfw_pad32(H2);
    float *X = s_mem, *A1 = X + D32 * kCfwLd, *A2 = A1 + H1p * kCfwLd;
    float *s_e = A2 + H2p * kCfwLd;                  // [2 H2p / 32][64]: the energy's partials per (block, lane half)
    float *s_mu = s_e + (H2p / 32) * 2 * kCfwRows;
    int *s_row = reinterpret_cast<int *>(s_mu + ((K + 3) & ~3));   // [64]: the tile's rows, -1 beyond the list
    CfwNet net;
    net.W1 = weights; net.b1 = net.W1 + D * H1; net.W2 = net.b1 + H1; net.b2 = net.W2 + H1 * H2; net.W3 = net.b2 + H2;
    net.b3 = net.W3 + H2;
    net.D = D; net.H1 = H1; net.H2 = H2;
    for (int i = threadIdx.x; i < K; i += blockDim.x) s_mu[i] = mu[i];
    __syncthreads();

    const float c_exp = -1.4426950408889634f / gap; // exp(-d^2 / gap) = exp2(c_exp d^2)
    const float c_fc = CUT ? cutoff_slope(rc) : 0.f;
    const unsigned lane = threadIdx.x & 63u;
    const int wave = (int)(threadIdx.x >> 6), nwaves = (int)(blockDim.x >> 6);
    const unsigned ns = (NN + 63u) >> 6;            // slots per lane in use (wave-uniform)
    const unsigned n_tiles = (n + kCfwRows - 1) / kCfwRows;

    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        // 1. the tile's descriptors: one row per wave at a time
        for (int tr = wave; tr < kCfwRows; tr += nwaves) {
            const unsigned q = tile * kCfwRows + (unsigned)tr;
            float g_mine = 0.f;
            int row = -1;
            if (q < n) {   // wave-uniform
                row = (int)q;
                if constexpr (LIST) row = rows[q];
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
                g_mine = cfw_row_channels<CUT>(r, fc, ty, ns, lane, s_mu, K, T, c_exp);
            }
            if ((int)lane < D32) X[lane * kCfwLd + tr] = g_mine;   // (lanes in [D, D32) and rows beyond the list: zeros)
            if (lane == 0) s_row[tr] = row;
        }
        __syncthreads();

        // 2. forward
        cfw_stage<TANH, 0>(net, X, A1, A2, s_e, H1p / 32, wave, nwaves, lane);
        __syncthreads();
        cfw_stage<TANH, 1>(net, X, A1, A2, s_e, H2p / 32, wave, nwaves, lane);
        __syncthreads();

        // 3. backward, in place
        cfw_stage<TANH, 2>(net, X, A1, A2, s_e, H1p / 32, wave, nwaves, lane);
        __syncthreads();
        cfw_stage<TANH, 3>(net, X, A1, A2, s_e, D32 / 32, wave, nwaves, lane);
        __syncthreads();

        // 4. g [row][D]: consecutive threads, consecutive channels of a row; E from the partials, blocks and halves in order
        for (int idx = threadIdx.x; idx < kCfwRows * D; idx += blockDim.x) {
            const int tr = idx / D, c = idx - tr * D;
            const int row = s_row[tr];
            if (row >= 0) g[(size_t)(unsigned)row * D + c] = X[c * kCfwLd + tr];
        }
        if (threadIdx.x < kCfwRows) {
            const int row = s_row[threadIdx.x];
            if (row >= 0) {
                float e = 0.f;
                for (int part = 0; part < (H2p / 32) * 2; ++part) e += s_e[part * kCfwRows + threadIdx.x];
                energy[(unsigned)row] = e + net.b3[0];
            }
        }
        __syncthreads();   // (the next tile's phase 1 writes X and the rows)
    }
}

inline size_t cfw_lds(unsigned K, unsigned T, unsigned H1, unsigned H2) {
    const size_t lines = (size_t)cfw_pad32((int)(K * T)) + cfw_pad32((int)H1) + cfw_pad32((int)H2);
    return (lines * kCfwLd + (size_t)(cfw_pad32((int)H2) / 32) * 2 * kCfwRows + ((K + 3) & ~3u) + kCfwRows) * sizeof(float);
}

// waves of a block: two per 32-wide column block of the wider layer (an item is then one block and row half), 4 to 8
inline unsigned cfw_waves(unsigned H1, unsigned H2) {
    const unsigned ncb = (unsigned)cfw_pad32((int)(H1 > H2 ? H1 : H2)) / 32u;
    const unsigned w = 2u * ncb;
    return w < (unsigned)kCfwMinWaves ? kCfwMinWaves : (w > (unsigned)kCfwMaxWaves ? kCfwMaxWaves : w);
}

// a launch above 64 KiB of dynamic LDS needs the kernel's limit raised first (committee.hip's cmt_raise_lds)
template <typename F>
inline int cfw_raise_lds(F kernel, size_t lds) {
    if (lds > 64u * 1024u)
        HTF_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return HTF_OK;
}

} // namespace
} // namespace htf

extern "C" int htf_cfw_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types, unsigned H1,
                            unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap, float *d_g,
                            float *d_energy, const int *d_rows, unsigned n_rows, float r_cut, htf_stream stream) {
    using namespace htf;
    int rc = desc_check(d_nlist, nlist_dtype, B, NN, K, n_types, d_mu, gap, d_g, HTF_F32);
    if (rc != HTF_OK) return rc;
    HTF_REQUIRE(d_weights, "descriptor network: null weights");
    HTF_REQUIRE(H1 >= 1 && H1 <= (unsigned)kCfwMaxH && H2 >= 1 && H2 <= (unsigned)kCfwMaxH,
                "descriptor network: hidden widths %u, %u outside [1, %d]", H1, H2, kCfwMaxH);
    HTF_REQUIRE(activation == HTF_ACT_LINEAR || activation == HTF_ACT_TANH, "descriptor network: unknown activation %d", activation);
    if ((rc = desc_check_rows(B, n_rows, r_cut)) != HTF_OK) return rc;
    HTF_REQUIRE(B == 0 || d_energy, "descriptor network: null pointer");
    const size_t lds = cfw_lds(K, n_types, H1, H2);
    HTF_REQUIRE(lds <= (size_t)HTF_CFW_MAX_LDS_BYTES,
                "descriptor network: a tile of %u x %u x %u needs %zu bytes of LDS, above the %u bytes of one compute unit",
                K * n_types, H1, H2, lds, HTF_CFW_MAX_LDS_BYTES);
    if (n_rows == 0) return HTF_OK;
    const unsigned tiles = (n_rows + kCfwRows - 1) / kCfwRows;
    const unsigned grid = tiles < kDescMaxBlocks ? tiles : kDescMaxBlocks;
    const unsigned threads = 64u * cfw_waves(H1, H2);
    const hipStream_t s = (hipStream_t)stream;
    dispatch_flags([&](auto TANH, auto CUT, auto LIST, auto F64) {
        using IT = scalar_t<F64>;
        auto kernel = cfw_tile_kernel<TANH, CUT, LIST, IT>;
        if ((rc = cfw_raise_lds(kernel, lds)) != HTF_OK) return;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, s, (const typename Vec4<IT>::type *)d_nlist, d_rows, n_rows, NN,
                           d_weights, d_mu, (int)K, (int)n_types, (int)H1, (int)H2, gap, r_cut, d_g, d_energy);
    }, activation == HTF_ACT_TANH, r_cut > 0.0f, d_rows != nullptr, nlist_dtype == HTF_F64);
    if (rc != HTF_OK) return rc;
    return check_launch("cfw_tile_kernel");
}
