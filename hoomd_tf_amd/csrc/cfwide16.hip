// Pass 1 of the conservative forces for wide networks on the fp16 matrix pipe (include/htf_cfwide16.h,
// htf.DescriptorMLP(conservative=True, dense="split16")): g_i = dE_i/dG_i and E_i of every listed row, cfwide.hip's tile with every
// operand of the dense stack as x = hi + lo in fp16 and three partial products per step on v_mfma_f32_32x32x16_f16 (fp32
// accumulators), as pair_mlp.hip's HTF_MLP_SPLIT16 and mlp_train16.hip do for the pair network.
//
// One block works on a tile of 64 listed rows at a time (grid-stride over the tiles).  The tile's activations live in LDS as three
// images of two fp16 planes each (hi, then lo), one line per TILE ROW and the features along it:
//
//   X  [2][64][D32 + 8]   G, later g as fp32 [64][D32 + 8]      A1 [2][64][H1p + 8]   h1, later dz1      A2 [2][64][H2p + 8]   dz2
//
// (D32, H1p, H2p: the widths rounded up to multiples of 32; the features beyond a width hold zeros) -- the bytes of cfwide.hip's
// fp32 images.  Every layer is computed transposed as there, Z^T[feature][row] = W^T X^T: lane (p, h) = (lane & 31, lane >> 5)
// supplies A[i = p][k0 + 8 h .. + 7] (weights, from global memory, split in registers) and B[k0 + 8 h .. + 7][j = p], which is 8
// consecutive fp16 of ITS OWN tile row p: one 16-byte LDS read per part.  Its accumulator register v holds feature
// 8 (v >> 2) + 4 h + (v & 3) of tile row p, so an epilogue writes 4 consecutive features as one 8-byte store per part.
// The lines are 8 fp16 (16 bytes) longer than the padded width: a line is then an odd number of 16-byte units, and the 16 lanes
// that a 16-byte read serves at a time (consecutive tile rows, the same k) fall on 16 different units of the 256-byte bank row;
// it is the smallest padding that keeps the reads aligned.  The 8-byte stores of 32 consecutive rows then fall on 16 units of 8
// bytes, two lanes each: one store per four accumulator registers against one read per three instructions, left as it is.
//
// The weights stay fp32 in L2, unpadded and untransposed, the guard on the load (reads past a width return 0):
//   forward   A[i][k] = W[k][i]: eight loads, each over 32 consecutive floats of row k for the 32 lanes of a half;
//   backward  A[i][k] = W[i][k]: a run of 8 consecutive floats of the lane's own row i.
// A chunk of 16 k is: split the 8 weights loaded one chunk ahead (hi = fp16(w), lo = fp16(w - hi), round to nearest: split16() of
// mlp_train16.hip, pair by pair), read the B parts, issue the next chunk's loads, then lo_a hi_b, hi_a lo_b, hi_a hi_b for each row
// half (the small products first, as there).  A split weight feeds three instructions per row half.
//
// Phases of a tile, a block barrier between them (cfwide.hip's):
//   1. descriptor   G_i by the row kernel's own sums (cfw_row_channels, copied): the row kernel's bits, then split into X
//   2. forward      h1 = act(z1) split into A1; z2's epilogue forms h2, the lane's share of E_i in fp32, and S dz2 split into A2
//   3. backward     S dz1 = (W2 S dz2) act'(z1) over A1 in place (a lane writes its own elements only; act'(z1) waits in 16
//                   registers per row half from the forward epilogue, see c16_act: rebuilt as 1 - (hi + lo)^2 it missed the fp32
//                   stack's bound on saturated units); g = (W1 S dz1) / S as fp32 into X's bytes: g is never rounded through fp16
//   4. store        g [row][D] coalesced, E_i from the partials in fixed order + b3
// S is the power of two that puts the largest |W3| into [32, 64) (seed_scale, pair_mlp.h, times 32), found by every block from the
// weights it is given.  The backward operands are W3 act' and sums of them, act' <= 1 shrinks them layer by layer, and an fp16
// lo part below 2^-14 keeps an absolute step of 2^-24 instead of a relative one: with the largest |W3| in [1, 2) the 1 x 1 tanh
// network missed the fp32 stack's bound by a fifth, the error that of S dz1's lo parts.  The factor 32 leaves S dz1 inside
// fp16's range while a row of |W2| sums to less than 1 000.  S and 1 / S are exact.  An operand beyond fp16's range (|v| > 65504: activation "linear" and
// extreme weights) splits into hi = +-inf, lo = -+inf and its row's products into NaN: non-finite, never a wrong finite value.
//
// No atomics, no state between calls (w is stepped in place: nothing is cached), the same bits at every call.  Built with
// cfwide.o's flags.
#include "htf_cfwide16.h"
#include "desc_row.h"
#include "pair_mlp.h"

namespace htf {
namespace {

using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
using u32x4t = __attribute__((ext_vector_type(4))) unsigned;
#define HTF_MFMA_H(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)

constexpr int kC16Rows = 64;     // rows of a tile: two 32-row halves
constexpr int kC16Pad = 8;       // fp16 a line is longer than its padded width (see above)
constexpr int kC16MaxH = HTF_CFW16_MAX_H;
constexpr int kC16MinWaves = 4, kC16MaxWaves = 8;

__host__ __device__ constexpr int c16_pad32(int v) { return (v + 31) & ~31; }
__host__ __device__ constexpr int c16_ld(int width) { return c16_pad32(width) + kC16Pad; }             // fp16 per line
__host__ __device__ constexpr int c16_plane(int width) { return kC16Rows * c16_ld(width); }           // fp16 per plane

struct C16Net {
    const float *W1, *b1, *W2, *b2, *W3, *b3;   // global memory, Keras order
    int D, H1, H2;
    float scale, inv_scale;                     // S and 1 / S of the backward operands
};

// an image: its hi plane, the distance to the lo plane and between two lines, in fp16
struct C16Img {
    _Float16 *hi;
    int plane, ld;
};

// desc_rows' step 2 (desc_row.h) as cfwide.hip's cfw_row_channels has it, statement for statement: G from the lanes' kept
// slots.  Lane t*K + k returns channel k of type t, every other lane 0.
template <bool CUT>
__device__ __forceinline__ float c16_row_channels(const float (&r)[kDescSlots], const float (&fc)[kDescSlots], const int (&ty)[kDescSlots],
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

// h = act(z) as desc_act has it (the same bits) and s = act'(z).  For tanh s = 1 - h^2 = 4 e r^2 with e = exp(2 z), r = 1 / (1 + e):
// products only, so a saturated unit keeps the relative accuracy of its small derivative, where 1 - h h cancels (h carries an
// absolute error of 6e-8 as an fp32 number and of up to 1.2e-7 once rebuilt from fp16 parts; at |z| = 4 that is 1e-4 of s).  e is
// capped so that an overflowed exponential gives s = 0 and not inf 0, by a compare that lets a NaN through: a weight beyond fp16's
// range makes z a NaN, and h and s must say so.
template <bool TANH>
__device__ __forceinline__ void c16_act(float z, float &h, float &s) {
    if constexpr (!TANH) {
        h = z;
        s = 1.0f;
    } else {
        float e = __expf(2.0f * z);
        e = e > 1.0e30f ? 1.0e30f : e;   // (not fminf: a NaN z must stay a NaN, as in desc_act)
        const float r = __builtin_amdgcn_rcpf(1.0f + e);
        h = fmaf(-2.0f, r, 1.0f);
        s = 4.0f * (e * r) * r;
    }
}

// (a, b) = hi + lo, both fp16 and rounded to nearest, packed: v_cvt_pk_f16_f32, the residuals by v_fma_mix_f32 reading hi from its
// half of the packed register (mlp_train16.hip split16(), one pair).  The values pass through an empty asm first: hipcc otherwise
// folds the fma that produced them into the conversion (v_fma_mixlo_f16), next to the fp32 fma the residual still needs.
__device__ __forceinline__ void c16_split2(float a, float b, unsigned &hp, unsigned &lp) {
    asm("" : "+v"(a));
    asm("" : "+v"(b));
    hp = __builtin_bit_cast(unsigned, f16x2{(_Float16)a, (_Float16)b});
    float ra, rb;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(ra) : "v"(hp), "v"(a));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(rb) : "v"(hp), "v"(b));
    lp = __builtin_bit_cast(unsigned, f16x2{(_Float16)ra, (_Float16)rb});
}

__device__ __forceinline__ void c16_split8(const float (&a)[8], f16x8 &hi, f16x8 &lo) {
    u32x4t ph, pl;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned hp, lp;
        c16_split2(a[2 * j], a[2 * j + 1], hp, lp);
        ph[j] = hp;
        pl[j] = lp;
    }
    hi = __builtin_bit_cast(f16x8, ph);
    lo = __builtin_bit_cast(f16x8, pl);
}

// four consecutive features of one tile row, split, as one 8-byte store per part
__device__ __forceinline__ void c16_store4(const C16Img &img, int at, float a, float b, float c, float d) {
    uint2 h, l;
    c16_split2(a, b, h.x, l.x);
    c16_split2(c, d, h.y, l.y);
    *reinterpret_cast<uint2 *>(img.hi + at) = h;
    *reinterpret_cast<uint2 *>(img.hi + img.plane + at) = l;
}

// the 8 weights of lane (i, h) for the chunk at k0: k = k0 + 8 h + t.  TRANS: A[i][k] = W[i][k], W [n_i][n_k]; else A[i][k] =
// W[k][i], W [n_k][n_i].  Zeros beyond either width (and beyond the last chunk: the look-ahead of the loop below loads nothing).
template <bool TRANS>
__device__ __forceinline__ void c16_weights(float (&a)[8], const float *__restrict__ W, int n_i, int n_k, int i, int k0, int h) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int k = k0 + 8 * h + t;
        a[t] = 0.f;
        if (i < n_i && k < n_k) a[t] = TRANS ? W[i * n_k + k] : W[k * n_i + i];
    }
}

// acc[hf] += A B over all n_k (padded to 16; the image has its zeros there): A's row i from W, B from the image at `at`, this
// lane's tile row and its 8 h (row half hf is 32 lines on).  The weights are loaded a chunk ahead of their instructions.
template <int NH, bool TRANS>
__device__ __forceinline__ void c16_mm(f32x16 (&acc)[NH], const float *__restrict__ W, int n_i, int n_k, int i, const C16Img &img, int at,
                                       int h) {
    float raw[8];
    c16_weights<TRANS>(raw, W, n_i, n_k, i, 0, h);
    for (int k0 = 0; k0 < n_k; k0 += 16) {
        f16x8 ah, al, bh[NH], bl[NH];
        c16_split8(raw, ah, al);
#pragma unroll
        for (int hf = 0; hf < NH; ++hf) {
            const _Float16 *q = img.hi + at + 32 * hf * img.ld + k0;
            bh[hf] = *reinterpret_cast<const f16x8 *>(q);
            bl[hf] = *reinterpret_cast<const f16x8 *>(q + img.plane);
        }
        c16_weights<TRANS>(raw, W, n_i, n_k, i, k0 + 16, h);
#pragma unroll
        for (int hf = 0; hf < NH; ++hf) acc[hf] = HTF_MFMA_H(al, bh[hf], acc[hf]);
#pragma unroll
        for (int hf = 0; hf < NH; ++hf) acc[hf] = HTF_MFMA_H(ah, bl[hf], acc[hf]);
#pragma unroll
        for (int hf = 0; hf < NH; ++hf) acc[hf] = HTF_MFMA_H(ah, bh[hf], acc[hf]);
    }
}

// One 32-feature block cb of a stage, for NH row halves from hf0 on.  STAGE 0: h1 -> A1.  1: S dz2 -> A2 and the energy partials.
// 2: S dz1 -> A1 in place.  3: g -> X's bytes as fp32.  s1: act'(z1) of this lane's elements, written by stage 0 and read by stage
// 2, which the same lane of the same wave runs for the same block and row halves (c16_stage).
template <bool TANH, int STAGE, int NH>
__device__ __forceinline__ void c16_block(const C16Net &net, const C16Img &X, const C16Img &A1, const C16Img &A2, float *s_e,
                                          float (&s1)[2][16], int cb, int hf0, unsigned lane) {
    const int p = (int)(lane & 31u), h = (int)(lane >> 5);
    const int row = 32 * hf0 + p;       // this lane's tile row in the first of its halves
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
    if constexpr (STAGE == 0) c16_mm<NH, false>(acc, net.W1, net.H1, net.D, ia, X, row * X.ld + 8 * h, h);
    if constexpr (STAGE == 1) c16_mm<NH, false>(acc, net.W2, net.H2, net.H1, ia, A1, row * A1.ld + 8 * h, h);
    if constexpr (STAGE == 2) c16_mm<NH, true>(acc, net.W2, net.H1, net.H2, ia, A2, row * A2.ld + 8 * h, h);
    if constexpr (STAGE == 3) c16_mm<NH, true>(acc, net.W1, net.D, net.H1, ia, A1, row * A1.ld + 8 * h, h);

    if constexpr (STAGE == 0) {
#pragma unroll
        for (int hf = 0; hf < NH; ++hf)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float h1[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) c16_act<TANH>(acc[hf][4 * c + j], h1[j], s1[hf][4 * c + j]);
                c16_store4(A1, (row + 32 * hf) * A1.ld + f_base + 8 * c, h1[0], h1[1], h1[2], h1[3]);
            }
    } else if constexpr (STAGE == 1) {
        float w3[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) w3[v] = f_base + f0(v) < net.H2 ? net.W3[f_base + f0(v)] : 0.f;
#pragma unroll
        for (int hf = 0; hf < NH; ++hf) {
            float e = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float dz[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float h2, s2;
                    c16_act<TANH>(acc[hf][4 * c + j], h2, s2);
                    e = fmaf(h2, w3[4 * c + j], e);
                    dz[j] = w3[4 * c + j] * net.scale * s2;
                }
                c16_store4(A2, (row + 32 * hf) * A2.ld + f_base + 8 * c, dz[0], dz[1], dz[2], dz[3]);
            }
            s_e[(2 * cb + h) * kC16Rows + row + 32 * hf] = e;
        }
    } else if constexpr (STAGE == 2) {
#pragma unroll
        for (int hf = 0; hf < NH; ++hf)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                c16_store4(A1, (row + 32 * hf) * A1.ld + f_base + 8 * c, acc[hf][4 * c] * s1[hf][4 * c], acc[hf][4 * c + 1] * s1[hf][4 * c + 1],
                           acc[hf][4 * c + 2] * s1[hf][4 * c + 2], acc[hf][4 * c + 3] * s1[hf][4 * c + 3]);
    } else {
        float *Xf = reinterpret_cast<float *>(X.hi);   // [64][X.ld] fp32: the two planes' bytes
#pragma unroll
        for (int hf = 0; hf < NH; ++hf)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                *reinterpret_cast<float4 *>(Xf + (row + 32 * hf) * X.ld + f_base + 8 * c) =
                    make_float4(acc[hf][4 * c] * net.inv_scale, acc[hf][4 * c + 1] * net.inv_scale, acc[hf][4 * c + 2] * net.inv_scale,
                                acc[hf][4 * c + 3] * net.inv_scale);
    }
}

// The ncb column blocks of a stage over the block's waves (wave-uniform branches), cfwide.hip's cfw_stage.  A wave has at most
// one item per stage: either 2 ncb <= nwaves, or the launcher's block has 8 waves (c16_waves: twice the blocks of the wider
// layer, capped at 8) and ncb <= 256 / 32 -- so what stage 0 leaves in s1 is what stage 2 of the same wave needs.  (The loops
// run once or not at all; written as `if` the same code takes 256 registers and spills 34 to 42 of them.)
static_assert(kC16MaxH / 32 <= kC16MaxWaves, "one column block per wave at the most");
template <bool TANH, int STAGE>
__device__ __forceinline__ void c16_stage(const C16Net &net, const C16Img &X, const C16Img &A1, const C16Img &A2, float *s_e,
                                          float (&s1)[2][16], int ncb, int wave, int nwaves, unsigned lane) {
    if (2 * ncb <= nwaves) {
        for (int item = wave; item < 2 * ncb; item += nwaves) c16_block<TANH, STAGE, 1>(net, X, A1, A2, s_e, s1, item >> 1, item & 1, lane);
    } else {
        for (int cb = wave; cb < ncb; cb += nwaves) c16_block<TANH, STAGE, 2>(net, X, A1, A2, s_e, s1, cb, 0, lane);
    }
}

template <bool TANH, bool CUT, bool LIST, typename IT>
__global__ __launch_bounds__(64 * kC16MaxWaves) void cfw16_tile_kernel(const typename Vec4<IT>::type *__restrict__ nlist,
                                                                       const int *__restrict__ rows, unsigned n, unsigned NN,
                                                                       const float *__restrict__ weights, const float *__restrict__ mu,
                                                                       int K, int T, int H1, int H2, float gap, float rc,
                                                                       float *__restrict__ g, float *__restrict__ energy) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int D = K * T;
    const int H2p = c16_pad32(H2);
    C16Img X, A1, A2;
    X.hi = reinterpret_cast<_Float16 *>(s_raw);
    X.ld = c16_ld(D); X.plane = c16_plane(D);
    A1.hi = X.hi + 2 * X.plane;
    A1.ld = c16_ld(H1); A1.plane = c16_plane(H1);
    A2.hi = A1.hi + 2 * A1.plane;
    A2.ld = c16_ld(H2); A2.plane = c16_plane(H2);
    float *s_e = reinterpret_cast<float *>(A2.hi + 2 * A2.plane);   // [2 H2p / 32][64]: the energy's partials per (block, lane half)
    float *s_mu = s_e + (H2p / 32) * 2 * kC16Rows;
    int *s_row = reinterpret_cast<int *>(s_mu + ((K + 3) & ~3));     // [64]: the tile's rows, -1 beyond the list
    float *s_scale = reinterpret_cast<float *>(s_row + kC16Rows);    // S, 1 / S
    C16Net net;
    net.W1 = weights; net.b1 = net.W1 + D * H1; net.W2 = net.b1 + H1; net.b2 = net.W2 + H1 * H2; net.W3 = net.b2 + H2;
    net.b3 = net.W3 + H2;
    net.D = D; net.H1 = H1; net.H2 = H2;
    for (int i = threadIdx.x; i < K; i += blockDim.x) s_mu[i] = mu[i];
    if (threadIdx.x < 64) {   // the first wave: the largest |W3| (non-negative floats order as their bits; a NaN wins and S = 1)
        unsigned m = 0u;
        for (int f = (int)threadIdx.x; f < H2; f += 64) {
            const unsigned u = __float_as_uint(fabsf(net.W3[f]));
            m = u > m ? u : m;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned o = (unsigned)__shfl_xor((int)m, d);
            m = o > m ? o : m;
        }
        if (threadIdx.x == 0) {
            const float s = 32.0f * seed_scale(__uint_as_float(m));
            s_scale[0] = s;
            s_scale[1] = 1.0f / s;
        }
    }
    __syncthreads();
    net.scale = s_scale[0];
    net.inv_scale = s_scale[1];

    const float c_exp = -1.4426950408889634f / gap; // exp(-d^2 / gap) = exp2(c_exp d^2)
    const float c_fc = CUT ? cutoff_slope(rc) : 0.f;
    const unsigned lane = threadIdx.x & 63u;
    const int wave = (int)(threadIdx.x >> 6), nwaves = (int)(blockDim.x >> 6);
    const unsigned ns = (NN + 63u) >> 6;            // slots per lane in use (wave-uniform)
    const unsigned n_tiles = (n + kC16Rows - 1) / kC16Rows;
    const int D32 = c16_pad32(D);
    const float *Xf = reinterpret_cast<const float *>(X.hi);

    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        // 1. the tile's descriptors: one row per wave at a time
        for (int tr = wave; tr < kC16Rows; tr += nwaves) {
            const unsigned q = tile * kC16Rows + (unsigned)tr;
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
                g_mine = c16_row_channels<CUT>(r, fc, ty, ns, lane, s_mu, K, T, c_exp);
            }
            if ((int)lane < D32) {   // (lanes in [D, D32) and rows beyond the list: zeros)
                asm("" : "+v"(g_mine));
                const _Float16 hi = (_Float16)g_mine;
                X.hi[tr * X.ld + (int)lane] = hi;
                X.hi[X.plane + tr * X.ld + (int)lane] = (_Float16)(g_mine - (float)hi);
            }
            if (lane == 0) s_row[tr] = row;
        }
        __syncthreads();

        // 2. forward
        float s1[2][16];   // act'(z1) of this lane's elements, from stage 0 to stage 2
        c16_stage<TANH, 0>(net, X, A1, A2, s_e, s1, c16_pad32(H1) / 32, wave, nwaves, lane);
        __syncthreads();
        c16_stage<TANH, 1>(net, X, A1, A2, s_e, s1, H2p / 32, wave, nwaves, lane);
        __syncthreads();

        // 3. backward, in place
        c16_stage<TANH, 2>(net, X, A1, A2, s_e, s1, c16_pad32(H1) / 32, wave, nwaves, lane);
        __syncthreads();
        c16_stage<TANH, 3>(net, X, A1, A2, s_e, s1, D32 / 32, wave, nwaves, lane);
        __syncthreads();

        // 4. g [row][D]: consecutive threads, consecutive channels of a row; E from the partials, blocks and halves in order
        for (int idx = threadIdx.x; idx < kC16Rows * D; idx += blockDim.x) {
            const int tr = idx / D, c = idx - tr * D;
            const int row = s_row[tr];
            if (row >= 0) g[(size_t)(unsigned)row * D + c] = Xf[tr * X.ld + c];
        }
        if (threadIdx.x < kC16Rows) {
            const int row = s_row[threadIdx.x];
            if (row >= 0) {
                float e = 0.f;
                for (int part = 0; part < (H2p / 32) * 2; ++part) e += s_e[part * kC16Rows + threadIdx.x];
                energy[(unsigned)row] = e + net.b3[0];
            }
        }
        __syncthreads();   // (the next tile's phase 1 writes X and the rows)
    }
}

inline size_t c16_lds(unsigned K, unsigned T, unsigned H1, unsigned H2) {
    const size_t halves = 2u * (size_t)(c16_plane((int)(K * T)) + c16_plane((int)H1) + c16_plane((int)H2));
    return halves * 2u + ((size_t)(c16_pad32((int)H2) / 32) * 2 * kC16Rows + ((K + 3) & ~3u) + kC16Rows + 4) * sizeof(float);
}

// waves of a block: two per 32-wide column block of the wider layer (an item is then one block and row half), 4 to 8
inline unsigned c16_waves(unsigned H1, unsigned H2) {
    const unsigned ncb = (unsigned)c16_pad32((int)(H1 > H2 ? H1 : H2)) / 32u;
    const unsigned w = 2u * ncb;
    return w < (unsigned)kC16MinWaves ? kC16MinWaves : (w > (unsigned)kC16MaxWaves ? kC16MaxWaves : w);
}

// a launch above 64 KiB of dynamic LDS needs the kernel's limit raised first (cfwide.hip's cfw_raise_lds)
template <typename F>
inline int c16_raise_lds(F kernel, size_t lds) {
    if (lds > 64u * 1024u)
        HTF_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return HTF_OK;
}

} // namespace
} // namespace htf

extern "C" int htf_cfw16_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types, unsigned H1,
                              unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap, float *d_g,
                              float *d_energy, const int *d_rows, unsigned n_rows, float r_cut, htf_stream stream) {
    using namespace htf;
    int rc = desc_check(d_nlist, nlist_dtype, B, NN, K, n_types, d_mu, gap, d_g, HTF_F32);
    if (rc != HTF_OK) return rc;
    HTF_REQUIRE(d_weights, "descriptor network: null weights");
    HTF_REQUIRE(H1 >= 1 && H1 <= (unsigned)kC16MaxH && H2 >= 1 && H2 <= (unsigned)kC16MaxH,
                "descriptor network: hidden widths %u, %u outside [1, %d]", H1, H2, kC16MaxH);
    HTF_REQUIRE(activation == HTF_ACT_LINEAR || activation == HTF_ACT_TANH, "descriptor network: unknown activation %d", activation);
    if ((rc = desc_check_rows(B, n_rows, r_cut)) != HTF_OK) return rc;
    HTF_REQUIRE(B == 0 || d_energy, "descriptor network: null pointer");
    const size_t lds = c16_lds(K, n_types, H1, H2);
    HTF_REQUIRE(lds <= (size_t)HTF_CFW16_MAX_LDS_BYTES,
                "descriptor network: a tile of %u x %u x %u needs %zu bytes of LDS, above the %u bytes of one compute unit",
                K * n_types, H1, H2, lds, HTF_CFW16_MAX_LDS_BYTES);
    if (n_rows == 0) return HTF_OK;
    const unsigned tiles = (n_rows + kC16Rows - 1) / kC16Rows;
    const unsigned grid = tiles < kDescMaxBlocks ? tiles : kDescMaxBlocks;
    const unsigned threads = 64u * c16_waves(H1, H2);
    const hipStream_t s = (hipStream_t)stream;
    dispatch_flags([&](auto TANH, auto CUT, auto LIST, auto F64) {
        using IT = scalar_t<F64>;
        auto kernel = cfw16_tile_kernel<TANH, CUT, LIST, IT>;
        if ((rc = c16_raise_lds(kernel, lds)) != HTF_OK) return;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, s, (const typename Vec4<IT>::type *)d_nlist, d_rows, n_rows, NN,
                           d_weights, d_mu, (int)K, (int)n_types, (int)H1, (int)H2, gap, r_cut, d_g, d_energy);
    }, activation == HTF_ACT_TANH, r_cut > 0.0f, d_rows != nullptr, nlist_dtype == HTF_F64);
    if (rc != HTF_OK) return rc;
    return check_launch("cfw16_tile_kernel");
}
