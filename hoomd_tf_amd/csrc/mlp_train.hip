// Online force matching for the pair-MLP (FORCE_MODE::hoomd2tf, tensorflowcompute.py:347-370,
// SURVEY 8(f)-1): d(sum of squared residuals)/d(theta) for
//   pred_i = (F_i, E_i),  F_i = sum_j m_ij u'(r_ij) t_ij / r_ij,  E_i = 1/2 sum_j m_ij u(r_ij)
// with u = Dense(1) o act o Dense(H2) o act o Dense(H1) o RBF (layers.py:46-49 + Keras Dense).
// Keras gets this by back-propagating through tf.gradients (a double backward over
// [N, NN, K] / [N, NN, H] tensors).  Here it is ONE sweep over the pair vectors: with
//   a_ij = 2 m (res_i . t_ij) / r_ij,   b_ij = m res_iE,
// the loss gradient is d/dtheta sum_ij (a u' + b u); per pair that is a forward pass of
// the value and of its r-tangent, and ONE reverse pass over both.
//
// MI355X mapping: training runs every `period` steps, so this kernel favours exact fp32
// and simplicity over the matrix cores.  A wave walks the pairs of its rows one after the
// other; lane f owns hidden feature f: column f of W1/W2 and row f of W2 sit in its
// registers (160 VGPRs), activations of the other features arrive by v_readlane
// broadcasts (SGPR operands of the FMAs), and the weight gradients are outer-product
// accumulators dW1[k][f], dW2[f1][f] held in registers (96 VGPRs) for the whole kernel:
// no LDS, no atomics, one partial per wave, reduced in a fixed order (deterministic).
// ~900 VALU instructions per live pair; 4 waves per CU (one per SIMD, ~300 VGPRs).
#include <cstdlib>

#include "htf_common.h"
#include "dispatch.h"
#include "htf_internal.h"
#include "pair_mlp.h"

namespace htf {


template <bool TANH>
__device__ __forceinline__ float act_val(float z) {
    return act_fwd<TANH>(z);
}

__device__ __forceinline__ float bcast(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

#ifdef HTF_AB_VARIANTS // the first-generation VALU sweep: A/B builds only
template <bool TANH, typename IT>
__global__ __launch_bounds__(256, 1) void mlp_grad_kernel(const typename Vec4<IT>::type *__restrict__ nlist, unsigned B,
                                                          unsigned NN, const void *__restrict__ labels, int lab_f64,
                                                          const float4 *__restrict__ pred,
                                                          const float *__restrict__ theta, MlpDims dm,
                                                          const float *__restrict__ tab_c, float ginv,
                                                          float *__restrict__ partial, unsigned stride) {
    const int f = threadIdx.x & 63;
    const unsigned wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const unsigned nwaves = (gridDim.x * blockDim.x) >> 6;
    const bool in1 = f < dm.H1, in2 = f < dm.H2;

    float w1c[kK], w2c[kH], w2r[kH];
#pragma unroll
    for (int k = 0; k < kK; ++k) w1c[k] = (k < dm.K && in1) ? theta[k * dm.H1 + f] : 0.f;
#pragma unroll
    for (int a = 0; a < kH; ++a) {
        w2c[a] = (a < dm.H1 && in2) ? theta[dm.oW2 + a * dm.H2 + f] : 0.f;
        w2r[a] = (in1 && a < dm.H2) ? theta[dm.oW2 + f * dm.H2 + a] : 0.f;
    }
    const float b1f = in1 ? theta[dm.oB1 + f] : 0.f;
    const float b2f = in2 ? theta[dm.oB2 + f] : 0.f;
    const float w3f = in2 ? theta[dm.oW3 + f] : 0.f;
    // centre of RBF k = f & 31 from the operand-ordered table (pair_mlp.h: feature f0(v) + 4 h)
    const int kf = f & 31;
    const float cen = tab_c[((kf >> 2) & 1) * 16 + (kf & 3) + 4 * (kf >> 3)];

    float g1[kK], g2[kH];
#pragma unroll
    for (int k = 0; k < kK; ++k) g1[k] = 0.f;
#pragma unroll
    for (int a = 0; a < kH; ++a) g2[a] = 0.f;
    float gb1 = 0.f, gb2 = 0.f, gw3 = 0.f, gb3 = 0.f, loss = 0.f;

    for (unsigned row = wave; row < B; row += nwaves) {
        const float4 pr = pred[row];
        float lx, ly, lz, lw;
        if (lab_f64) {
            const double4 l = ((const double4 *)labels)[row];
            lx = (float)l.x; ly = (float)l.y; lz = (float)l.z; lw = (float)l.w;
        } else {
            const float4 l = ((const float4 *)labels)[row];
            lx = l.x; ly = l.y; lz = l.z; lw = l.w;
        }
        const float rx = pr.x - lx, ry = pr.y - ly, rz = pr.z - lz, re = pr.w - lw;
        loss += rx * rx + ry * ry + rz * rz + re * re;
        const typename Vec4<IT>::type *rp = nlist + (size_t)row * NN;
        for (unsigned j = 0; j < NN; ++j) {
            const auto v = load_stream(&rp[j]);
            const float tx = (float)v.x + kNormDelta, ty = (float)v.y + kNormDelta, tz = (float)v.z + kNormDelta;
            const float r = sqrtf(tx * tx + ty * ty + tz * tz);
            if (!(r > kRinvDelta)) continue; // padded slot (wave-uniform)
            const float a = 2.0f * (rx * tx + ry * ty + rz * tz) / r;
            const float b = re;
            const float d = r - cen;
            const float phi = __expf(-d * d * ginv);
            const float dphi = -2.0f * d * ginv * phi;
            // value and r-tangent, layer 1
            float z1 = b1f, zd1 = 0.f;
#pragma unroll
            for (int k = 0; k < kK; ++k) {
                z1 = fmaf(bcast(phi, k), w1c[k], z1);
                zd1 = fmaf(bcast(dphi, k), w1c[k], zd1);
            }
            const float h1 = act_val<TANH>(z1);
            const float s1 = TANH ? 1.0f - h1 * h1 : 1.0f;
            const float hd1 = s1 * zd1;
            float z2 = b2f, zd2 = 0.f;
#pragma unroll
            for (int k = 0; k < kH; ++k) {
                z2 = fmaf(bcast(h1, k), w2c[k], z2);
                zd2 = fmaf(bcast(hd1, k), w2c[k], zd2);
            }
            const float h2 = act_val<TANH>(z2);
            const float s2 = TANH ? 1.0f - h2 * h2 : 1.0f;
            const float hd2 = s2 * zd2;
            // reverse over S = a u' + b u  (u = w3 . h2 + b3, u' = w3 . hd2)
            gw3 += b * h2 + a * hd2;
            gb3 += b;
            const float hb2 = b * w3f, hdb2 = a * w3f;
            const float c2 = TANH ? -2.0f * h2 * s2 : 0.f; // act''(z2)
            const float zb2 = hb2 * s2 + hdb2 * c2 * zd2;
            const float zdb2 = hdb2 * s2;
            gb2 += zb2;
            float hb1 = 0.f, hdb1 = 0.f;
#pragma unroll
            for (int k = 0; k < kH; ++k) {
                hb1 = fmaf(w2r[k], bcast(zb2, k), hb1);
                hdb1 = fmaf(w2r[k], bcast(zdb2, k), hdb1);
            }
            const float c1 = TANH ? -2.0f * h1 * s1 : 0.f;
            const float zb1 = hb1 * s1 + hdb1 * c1 * zd1;
            const float zdb1 = hdb1 * s1;
            gb1 += zb1;
            // outer products: dW2[f1][f] += h1[f1] zb2[f] + hd1[f1] zdb2[f];  dW1[k][f] likewise
#pragma unroll
            for (int k = 0; k < kH; ++k) g2[k] = fmaf(bcast(h1, k), zb2, fmaf(bcast(hd1, k), zdb2, g2[k]));
#pragma unroll
            for (int k = 0; k < kK; ++k) g1[k] = fmaf(bcast(phi, k), zb1, fmaf(bcast(dphi, k), zdb1, g1[k]));
        }
    }
    float *out = partial + (size_t)wave * stride;
    if (f == 0) {
        out[0] = loss;
        out[1 + dm.oB3] = gb3;
    }
#pragma unroll
    for (int k = 0; k < kK; ++k)
        if (k < dm.K && in1) out[1 + k * dm.H1 + f] = g1[k];
#pragma unroll
    for (int a = 0; a < kH; ++a)
        if (a < dm.H1 && in2) out[1 + dm.oW2 + a * dm.H2 + f] = g2[a];
    if (in1) out[1 + dm.oB1 + f] = gb1;
    if (in2) {
        out[1 + dm.oB2 + f] = gb2;
        out[1 + dm.oW3 + f] = gw3;
    }
}

#endif // HTF_AB_VARIANTS

// ------------------------------------------------------------------ matrix-core version (fp32)
// The same sweep on the MFMA units.  Layers are computed transposed as in pair_mlp.hip
// (features on accumulator rows, a tile of 32 pairs on the lanes) for the value chain, its
// r-tangent chain and the one reverse pass over both (320 MFMAs per tile).  The weight
// gradients are contractions over PAIRS,
//     dW2[f1][f2] += sum_p h1[f1][p] zb2[f2][p] + hd1[f1][p] zdb2[f2][p]     (dW1 likewise),
// i.e. MFMAs whose k index is the pair: both operands are needed as [feature][pair] rows.
// Each wave publishes its tile's blocks through LDS (row stride 36 floats: conflict-free
// ds_write_b32 by pair, ds_read_b128 by feature; k order p = 16 h + t on both operands) and
// the four waves of a block split the accumulators: wave w owns the (w>>1, w&1) 32x32 block
// of dW2 over all four tiles and the (w&1) block of dW1 over two of them, so a wave carries
// 32 accumulator registers instead of 96.  192 MFMAs per tile in this phase; 8 block
// barriers per round.  Bias / w3 gradients ride along on the VALU.  One partial per block,
// combined in a fixed order -> deterministic.
// Measured alternative: the same sweep with v_mfma_f32_16x16x4_f32 and 16-pair tiles (every
// per-wave array half the size, 242 VGPRs, eight waves = two per SIMD on a CU) was built and is
// correct, but ran 11.5 ms against 11.05 ms: the block-wide barriers keep both waves of a SIMD
// in the same phase, so one wave's VALU/LDS work does not land under the other's MFMAs.  Two
// independently scheduled 4-wave blocks per CU would, but need 166 KB of LDS.
constexpr int kPS = 36;         // published row stride (floats)
constexpr int kPB = 32 * kPS;   // one published 32 x 32 block
constexpr int kSlots = 6;       // per wave: A0 A1 | B0 B1 | phi phid  (108 KB + 49 KB of images: one block per CU)

__device__ __forceinline__ void mfma_pair(f32x16 &acc0, f32x16 &acc1, const float *img, unsigned lane,
                                          const f32x16 &p0, const f32x16 &p1) {
    const float4 *p = reinterpret_cast<const float4 *>(img) + lane;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 w = p[g * 64];
        acc0 = HTF_MFMA(w.x, p0[4 * g + 0], acc0);
        acc1 = HTF_MFMA(w.x, p1[4 * g + 0], acc1);
        acc0 = HTF_MFMA(w.y, p0[4 * g + 1], acc0);
        acc1 = HTF_MFMA(w.y, p1[4 * g + 1], acc1);
        acc0 = HTF_MFMA(w.z, p0[4 * g + 2], acc0);
        acc1 = HTF_MFMA(w.z, p1[4 * g + 2], acc1);
        acc0 = HTF_MFMA(w.w, p0[4 * g + 3], acc0);
        acc1 = HTF_MFMA(w.w, p1[4 * g + 3], acc1);
    }
}

__device__ __forceinline__ void publish(float *blk, unsigned p, unsigned h, const f32x16 &a) {
#pragma unroll
    for (int v = 0; v < 16; ++v) blk[(f0(v) + 4 * h) * kPS + p] = a[v];
}

__device__ __forceinline__ f32x16 load_op(const float *blk, unsigned i, unsigned h) {
    const float4 *q = reinterpret_cast<const float4 *>(blk + i * kPS + 16 * h);
    const float4 a = q[0], b = q[1], c = q[2], d = q[3];
    f32x16 r;
    r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w;
    r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
    r[8] = c.x; r[9] = c.y; r[10] = c.z; r[11] = c.w;
    r[12] = d.x; r[13] = d.y; r[14] = d.z; r[15] = d.w;
    return r;
}

__device__ __forceinline__ float sum16(const f32x16 &a) {
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) s += a[v];
    return s;
}

__device__ __forceinline__ void outer16(f32x16 &acc, const f32x16 &A, const f32x16 &Bm) {
#pragma unroll
    for (int t = 0; t < 16; ++t) acc = HTF_MFMA(A[t], Bm[t], acc);
}



// FUSED (ntiles in {1, 2, 4}, i.e. NN <= 64 or 97..128): the block also forms the row's
// predicted (F_i, E_i) from the value/tangent outputs it has in hand, so the separate
// evaluator pass is skipped; `pred_out` (nullable) receives the prediction.
template <bool TANH, typename IT, bool FUSED>
__global__ __launch_bounds__(256, 1) void mlp_grad_mfma_kernel(const typename Vec4<IT>::type *__restrict__ nlist,
                                                               unsigned B, unsigned NN,
                                                               const void *__restrict__ labels, int lab_f64,
                                                               const float4 *__restrict__ pred,
                                                               float4 *__restrict__ pred_out,
                                                               const float *__restrict__ images, MlpDims dm, float gap,
                                                               float *__restrict__ partial, unsigned stride) {
    using I = Img<false>;
    __shared__ __attribute__((aligned(16))) float lds[I::Floats];
    __shared__ __attribute__((aligned(16))) float pub[4 * kSlots * kPB];
    __shared__ int live_flag[4];
    __shared__ float4 rowsum[4];
    {
        const float4 *src = reinterpret_cast<const float4 *>(images);
        float4 *dst = reinterpret_cast<float4 *>(lds);
        for (int i = threadIdx.x; i < I::Floats / 4; i += blockDim.x) dst[i] = src[i];
    }
    __syncthreads();

    const unsigned lane = threadIdx.x & 63u;
    const unsigned p = lane & 31u, h = lane >> 5;
    const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned ntiles = (NN + 31) / 32;
    const unsigned long long U = (unsigned long long)B * ntiles;
    // unit -> (row, tile).  FUSED launches have 1, 2 or 4 tiles per row: a shift and a mask instead of
    // 64-bit divisions (five per trip, each a ~100-instruction emulation)
    const unsigned tsh = ntiles == 4 ? 2u : (ntiles == 2 ? 1u : 0u);
    auto row_of = [&](unsigned long long u) { return FUSED ? (unsigned)(u >> tsh) : (unsigned)(u / ntiles); };
    auto tile_of = [&](unsigned long long u) { return FUSED ? (unsigned)u & (ntiles - 1u) : (unsigned)(u % ntiles); };
    const float ginv = 1.0f / gap;
    float *mine = pub + w * kSlots * kPB;

    f32x16 acc2 = zero16(), acc1 = zero16();
    f32x16 gw3[2] = {zero16(), zero16()};
    float gb1 = 0.f, gb2 = 0.f, gb3 = 0.f, loss = 0.f;

    for (unsigned long long base = (unsigned long long)blockIdx.x * 4; base < U; base += (unsigned long long)gridDim.x * 4) {
        const unsigned long long u = base + w;
        const bool valid = u < U;
        const unsigned row = valid ? row_of(u) : 0u, tile = valid ? tile_of(u) : 0u;
        const unsigned slot = tile * 32 + p;
        float x = 0.f, y = 0.f, z = 0.f;
        if (valid && slot < NN) {
            const auto v = load_stream(&nlist[(size_t)row * NN + slot]);
            x = (float)v.x; y = (float)v.y; z = (float)v.z;
        }
        const float tx = x + kNormDelta, ty = y + kNormDelta, tz = z + kNormDelta;
        const float r = sqrtf(tx * tx + ty * ty + tz * tz);
        const bool m = valid && slot < NN && r > kRinvDelta;
        const bool live = __ballot(m) != 0ull;

        // written and read only under `live` (wave-uniform): no initialisation -- twelve tiles of v_mov 0
        // per trip are VALU time the fp32 MFMAs cannot hide (pair_mlp.hip)
        f32x16 h1[2], hd1[2];
        f32x16 q2[2], qd2[2]; // zb2, zdb2
        f32x16 q1[2], qd1[2]; // zb1, zdb1
        float4 part = make_float4(0.f, 0.f, 0.f, 0.f); // this tile's share of (F_i, E_i)
        if (live) {
            // ---- value + r-tangent, forward.  phi / phid go to LDS at once (needed again only
            // for dW1 at the end of the round)
            f32x16 phi, phid;
            {
                const f32x16 cen = load_tab(lds + I::TabC, 0, h);
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const float d = r - cen[v];
                    phi[v] = __expf(-(d * d) * ginv);
                    phid[v] = -2.0f * d * ginv * phi[v];
                }
            }
            publish(mine + 4 * kPB, p, h, phi);
            publish(mine + 5 * kPB, p, h, phid);
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                f32x16 zz = load_tab(lds + I::TabB1, nb, h), zd = zero16();
                mfma_pair(zz, zd, lds + I::L1 + nb * I::BS, lane, phi, phid);
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const float hv = act_fwd<TANH>(zz[v]);
                    h1[nb][v] = hv;
                    hd1[nb][v] = TANH ? (1.0f - hv * hv) * zd[v] : zd[v];
                }
            }
            float upart = 0.f, dpart = 0.f;
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                f32x16 zz = load_tab(lds + I::TabB2, nb, h), zd = zero16();
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) mfma_pair(zz, zd, lds + I::L2 + (nb * 2 + kb) * I::BS, lane, h1[kb], hd1[kb]);
                const f32x16 w3 = load_tab(lds + I::TabW3, nb, h);
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const float hv = act_fwd<TANH>(zz[v]);
                    const float hdv = TANH ? (1.0f - hv * hv) * zd[v] : zd[v];
                    q2[nb][v] = hv;   // h2  (becomes zb2 below)
                    qd2[nb][v] = hdv; // hd2 (becomes zdb2)
                    upart = fmaf(hv, w3[v], upart);
                    dpart = fmaf(hdv, w3[v], dpart);
                }
            }
            if (FUSED) { // u = w3 . h2 + b3, u' = w3 . hd2: the prediction itself (pair_mlp.hip)
                const float uu = sum_xor32(upart) + lds[I::TabB3];
                const float du = sum_xor32(dpart);
                if (m && h == 0) {
                    const float c = du / r;
                    part = make_float4(c * tx, c * ty, c * tz, 0.5f * uu);
                }
            }
        }
        // ---- residual of this wave's row
        float4 rs;
        if (FUSED) {
            // ntiles in {1, 2, 4}: the row's tiles all sit in this round; sum them in wave order
            part.x = group_sum<64>(part.x);
            part.y = group_sum<64>(part.y);
            part.z = group_sum<64>(part.z);
            part.w = group_sum<64>(part.w);
            if (lane == 0) rowsum[w] = part;
            __syncthreads();
            float4 F = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (unsigned t = 0; t < 4; ++t) {
                const unsigned long long ut = base + t;
                if (ut < U && row_of(ut) == row) {
                    const float4 q = rowsum[t];
                    F.x += q.x; F.y += q.y; F.z += q.z; F.w += q.w;
                }
            }
            if (pred_out && valid && tile == 0 && lane == 0) pred_out[row] = F;
            float lx, ly, lz, lw;
            if (lab_f64) {
                const double4 l = ((const double4 *)labels)[row];
                lx = (float)l.x; ly = (float)l.y; lz = (float)l.z; lw = (float)l.w;
            } else {
                const float4 l = ((const float4 *)labels)[row];
                lx = l.x; ly = l.y; lz = l.z; lw = l.w;
            }
            rs = make_float4(F.x - lx, F.y - ly, F.z - lz, F.w - lw);
        } else {
            rs = residual(pred, labels, lab_f64, row);
        }
        if (valid && tile == 0 && lane == 0) loss += rs.x * rs.x + rs.y * rs.y + rs.z * rs.z + rs.w * rs.w;
        if (live) {
            // ---- reverse seed: S = a u' + b u
            const float aq = m ? 2.0f * (rs.x * tx + rs.y * ty + rs.z * tz) / r : 0.f;
            const float bq = m ? rs.w : 0.f;
            if (h == 0) gb3 += bq;
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const f32x16 w3 = load_tab(lds + I::TabW3, nb, h);
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const float hv = q2[nb][v], hdv = qd2[nb][v];
                    const float s2 = TANH ? 1.0f - hv * hv : 1.0f;
                    gw3[nb][v] += bq * hv + aq * hdv;
                    const float hb = bq * w3[v], hdb = aq * w3[v];
                    q2[nb][v] = TANH ? hb * s2 - 2.0f * hdb * hv * hdv : hb; // zb2
                    qd2[nb][v] = hdb * s2;                                     // zdb2
                }
            }
        }
        // ---- weight gradients: contractions over the pairs of the block's four tiles
        if (lane == 0) live_flag[w] = live ? 1 : 0;
        // D1: dW2 += h1 (x) zb2
        if (live) {
            publish(mine + 0 * kPB, p, h, h1[0]);
            publish(mine + 1 * kPB, p, h, h1[1]);
            publish(mine + 2 * kPB, p, h, q2[0]);
            publish(mine + 3 * kPB, p, h, q2[1]);
        }
        __syncthreads();
        const unsigned f1b = w >> 1, f2b = w & 1u;
#pragma unroll 1
        for (unsigned t = 0; t < 4; ++t) {
            if (!live_flag[t]) continue;
            const float *src = pub + t * kSlots * kPB;
            const f32x16 A = load_op(src + f1b * kPB, p, h), Bm = load_op(src + (2 + f2b) * kPB, p, h);
            outer16(acc2, A, Bm);
            if (f1b == 0) gb2 += sum16(Bm);
        }
        __syncthreads();
        // D2: dW2 += hd1 (x) zdb2
        if (live) {
            publish(mine + 0 * kPB, p, h, hd1[0]);
            publish(mine + 1 * kPB, p, h, hd1[1]);
            publish(mine + 2 * kPB, p, h, qd2[0]);
            publish(mine + 3 * kPB, p, h, qd2[1]);
        }
        __syncthreads();
#pragma unroll 1
        for (unsigned t = 0; t < 4; ++t) {
            if (!live_flag[t]) continue;
            const float *src = pub + t * kSlots * kPB;
            const f32x16 A = load_op(src + f1b * kPB, p, h), Bm = load_op(src + (2 + f2b) * kPB, p, h);
            outer16(acc2, A, Bm);
        }
        __syncthreads();
        if (live) {
            // ---- reverse through layer 2: (hb1, hdb1) = W2 (zb2, zdb2), then through act at z1
#pragma unroll
            for (int fb = 0; fb < 2; ++fb) {
                f32x16 hb = zero16(), hdb = zero16();
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) mfma_pair(hb, hdb, lds + I::B2 + (fb * 2 + kb) * I::BS, lane, q2[kb], qd2[kb]);
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const float hv = h1[fb][v];
                    const float s1 = TANH ? 1.0f - hv * hv : 1.0f;
                    q1[fb][v] = TANH ? hb[v] * s1 - 2.0f * hdb[v] * hv * hd1[fb][v] : hb[v]; // zb1
                    qd1[fb][v] = hdb[v] * s1;                                                  // zdb1
                }
            }
                }
        // D3: dW1 += phi (x) zb1  (wave w: feature block w&1, tiles 2(w>>1), 2(w>>1)+1)
        if (live) {
            publish(mine + 2 * kPB, p, h, q1[0]);
            publish(mine + 3 * kPB, p, h, q1[1]);
        }
        __syncthreads();
#pragma unroll 1
        for (unsigned t = 2 * (w >> 1); t < 2 * (w >> 1) + 2; ++t) {
            if (!live_flag[t]) continue;
            const float *src = pub + t * kSlots * kPB;
            const f32x16 A = load_op(src + 4 * kPB, p, h), Bm = load_op(src + (2 + (w & 1u)) * kPB, p, h);
            outer16(acc1, A, Bm);
            gb1 += sum16(Bm);
        }
        __syncthreads();
        // D4: dW1 += phid (x) zdb1
        if (live) {
            publish(mine + 2 * kPB, p, h, qd1[0]);
            publish(mine + 3 * kPB, p, h, qd1[1]);
        }
        __syncthreads();
#pragma unroll 1
        for (unsigned t = 2 * (w >> 1); t < 2 * (w >> 1) + 2; ++t) {
            if (!live_flag[t]) continue;
            const float *src = pub + t * kSlots * kPB;
            const f32x16 A = load_op(src + 5 * kPB, p, h), Bm = load_op(src + (2 + (w & 1u)) * kPB, p, h);
            outer16(acc1, A, Bm);
        }
        __syncthreads();
    }

    // ---- block partial in LDS, waves in a fixed order
    float *red = pub; // 1 + P <= 6338 floats
    for (unsigned c = threadIdx.x; c < stride; c += blockDim.x) red[c] = 0.f;
    __syncthreads();
    // gw3: sum over the 32 pairs of each lane half
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            float s = gw3[b][v];
            s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4);
            s += __shfl_xor(s, 8); s += __shfl_xor(s, 16);
            gw3[b][v] = s;
        }
    gb1 = sum_xor32(gb1);
    gb2 = sum_xor32(gb2);
    gb3 = group_sum<64>(gb3);
    for (unsigned turn = 0; turn < 4; ++turn) {
        if (w == turn) {
            // acc2: lane (j, h) register v = dW2[32 (w>>1) + f0(v) + 4h][32 (w&1) + j]
            const int f2 = 32 * (int)(w & 1u) + (int)p;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int f1 = 32 * (int)(w >> 1) + f0(v) + 4 * (int)h;
                if (f1 < dm.H1 && f2 < dm.H2) red[1 + dm.oW2 + f1 * dm.H2 + f2] += acc2[v];
            }
            // acc1: lane (j, h) register v = dW1[f0(v) + 4h][32 (w&1) + j]
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int k = f0(v) + 4 * (int)h;
                if (k < dm.K && f2 < dm.H1) red[1 + k * dm.H1 + f2] += acc1[v];
            }
            if (h == 0 && f2 < dm.H1) red[1 + dm.oB1 + f2] += gb1;
            if (h == 0 && (w >> 1) == 0 && f2 < dm.H2) red[1 + dm.oB2 + f2] += gb2;
            if (p == 0) {
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int f = 32 * b + f0(v) + 4 * (int)h;
                        if (f < dm.H2) red[1 + dm.oW3 + f] += gw3[b][v];
                    }
            }
            if (lane == 0) {
                red[1 + dm.oB3] += gb3;
                red[0] += loss;
            }
        }
        __syncthreads();
    }
    float *out = partial + (size_t)blockIdx.x * stride;
    for (unsigned c = threadIdx.x; c < stride; c += blockDim.x) out[c] = red[c];
}

// accum[c] = sum over the block partials, fixed order; columns >= 1 (the gradient) times 1 / S when the sweep scaled its seeds.
// 64 columns x 8 slices of the partials per workgroup (a thread per column walking all 256 partials took 62 us, 2 % of the sweep):
// slice sums in fixed order, slices combined in fixed order -> deterministic.
constexpr unsigned kRedSlices = 8;
// ``windows`` > 1 (the split16 sweep): `partial` holds that many groups of nwaves partials, group w scaled by
// seed_scale(*resid_max) 2^(kWindowBits w); each group is summed as above, unscaled, and the groups added in order.
__global__ __launch_bounds__(64 * kRedSlices) void mlp_reduce_partials_kernel(const float *__restrict__ partial, unsigned nwaves, unsigned stride,
                                                                              unsigned ncols, float *__restrict__ accum,
                                                                              const float *__restrict__ resid_max, int windows) {
    __shared__ float part[kRedSlices][64];
    const unsigned col = threadIdx.x & 63u, slice = threadIdx.x >> 6;
    const unsigned c = blockIdx.x * 64 + col;
    const unsigned per = (nwaves + kRedSlices - 1) / kRedSlices;
    const unsigned w0 = slice * per, w1 = w0 + per < nwaves ? w0 + per : nwaves;
    float total = 0.f;
    for (int win = 0; win < windows; ++win) {
        const float *pw = partial + (size_t)win * nwaves * stride;
        float s = 0.f;
        if (c < ncols)
            for (unsigned w = w0; w < w1; ++w) s += pw[(size_t)w * stride + c];
        __syncthreads();
        part[slice][col] = s;
        __syncthreads();
        if (slice == 0 && c < ncols) {
#pragma unroll
            for (unsigned k = 1; k < kRedSlices; ++k) s += part[k][col];
            if (resid_max && c > 0) {
                const float R = *resid_max;
                const float S = (R > 0.f && R < 3.0e38f) ? ldexpf(seed_scale(R), kWindowBits * win) : 1.0f;
                s *= 1.0f / S; // a power of two: exact
            }
            total += s;
        }
    }
    if (slice == 0 && c < ncols) accum[c] = total;
}

// partial slots of a launch: the VALU kernel writes one per wave (n_cu x 4, or the rows rounded up to a multiple of 4), the
// matrix-core kernels one per workgroup -- up to n_cu of them, sized by the launch's UNITS (rows x tiles for the fp32 sweep:
// a short batch of long rows has more workgroups than rows / 4; round 4: the scratch had been sized by the rows alone)
static unsigned train_waves(const MlpDevice *m, unsigned B) {
    unsigned w = (unsigned)m->n_cu * 4u;
    if (w > B) w = (B + 3u) & ~3u;
    return w;
}
static unsigned train_slots(const MlpDevice *m, unsigned B, unsigned NN) {
    const unsigned long long units = (unsigned long long)B * ((NN + 31) / 32);
    const unsigned long long blocks = (units + 3) / 4 < (unsigned long long)m->n_cu ? (units + 3) / 4 : (unsigned long long)m->n_cu;
    const unsigned w = train_waves(m, B);
    return blocks > w ? (unsigned)blocks : w;
}

static unsigned train_stride(const MlpDevice *m) { return ((unsigned)m->num_params() + 1u + 3u) & ~3u; }

// block partials | prediction [B, 4] (when the caller wants none back) | the largest residual of the launch (1 float + pad)
size_t mlp_train_scratch_floats(const MlpDevice *m, unsigned B, unsigned NN) {
    if (!m) return 0;
    // (the split16 sweep writes one group of partials per residual window)
    const size_t groups = m->precision == HTF_MLP_SPLIT16 ? (size_t)kTrainWindows : 1;
    return groups * train_slots(m, B, NN) * train_stride(m) + (size_t)B * 4 + 4;
}

int mlp_train_grad(const MlpDevice *m, const void *nlist, int in_dtype, unsigned B, unsigned NN, const void *labels,
                   int lab_f64, void *pred, float *accum, float *scratch, hipStream_t stream) {
    HTF_REQUIRE(m, "pair-MLP: null potential");
    const unsigned nw = train_waves(m, B), stride = train_stride(m);
    const unsigned slots = train_slots(m, B, NN) * (m->precision == HTF_MLP_SPLIT16 ? (unsigned)kTrainWindows : 1u);
    (void)nw; // (the VALU kernel's wave count: variants builds)
    float *partial = scratch;
    float4 *predbuf = pred ? (float4 *)pred : (float4 *)(scratch + (size_t)slots * stride);
    float *resid_max = scratch + (size_t)slots * stride + (size_t)B * 4;
    const unsigned ntiles = (NN + 31) / 32;
    MlpDims dm{m->K, m->H1, m->H2, m->off_b1(), m->off_W2(), m->off_b2(), m->off_W3(), m->off_b3()};
    const bool th = m->act == HTF_ACT_TANH;
    const unsigned ncols = (unsigned)m->num_params() + 1u;
    int rc = HTF_OK;
#ifdef HTF_AB_VARIANTS // A/B builds only (make variants): the first-generation kernels stay selectable; read per call, tests toggle them
    const bool force_valu = getenv("HTF_MLP_TRAIN_VALU") != nullptr;
    const bool no_fuse = getenv("HTF_MLP_TRAIN_NOFUSE") != nullptr;
    const bool force_fp32 = getenv("HTF_MLP_TRAIN_FP32") != nullptr;
#else
    constexpr bool force_valu = false, no_fuse = false, force_fp32 = false;
#endif
    // split16 potentials: the sweep runs on the fp16 pipeline from the evaluator's own images, every wave on its own
    // (mlp_grad_tr16_kernel); every other precision trains on its fp32 image set with the fp32 MFMA
    if (m->precision == HTF_MLP_SPLIT16 && !force_fp32 && !force_valu) {
        unsigned nblk = 0;
        rc = mlp_train_grad16(m, nlist, in_dtype, B, NN, labels, lab_f64, predbuf, partial, stride, resid_max, &nblk, stream);
        if (rc != HTF_OK) return rc;
        hipLaunchKernelGGL(mlp_reduce_partials_kernel, dim3((ncols + 63) / 64), dim3(64 * kRedSlices), 0, stream, partial, nblk, stride,
                           ncols, accum, resid_max, kTrainWindows);
        return check_launch("mlp_reduce_partials_kernel");
    }
    const bool fused = !force_valu && !no_fuse && (ntiles == 1 || ntiles == 2 || ntiles == 4);
    if (!fused) {
        rc = mlp_eval(m, nlist, in_dtype, B, NN, predbuf, HTF_F32, nullptr, stream);
        if (rc != HTF_OK) return rc;
    }
    if (!force_valu) {
        const unsigned long long units = (unsigned long long)B * ntiles;
        unsigned nblk = (unsigned)m->n_cu;
        if ((unsigned long long)nblk * 4 > units) nblk = (unsigned)((units + 3) / 4);
        dispatch_flags([&](auto TANH, auto F64, auto FUSED) {
            using IT = scalar_t<F64>;
            hipLaunchKernelGGL((mlp_grad_mfma_kernel<TANH, IT, FUSED>), dim3(nblk), dim3(256), 0, stream, (const typename Vec4<IT>::type *)nlist,
                               B, NN, labels, lab_f64, predbuf, (float4 *)pred, m->train_images, dm, m->gap, partial, stride);
        }, th, in_dtype != HTF_F32, fused);
        rc = check_launch("mlp_grad_mfma_kernel");
        if (rc != HTF_OK) return rc;
        hipLaunchKernelGGL(mlp_reduce_partials_kernel, dim3((ncols + 63) / 64), dim3(64 * kRedSlices), 0, stream, partial, nblk, stride,
                           ncols, accum, (const float *)nullptr, 1);
        return check_launch("mlp_reduce_partials_kernel");
    }
#ifdef HTF_AB_VARIANTS
    const float *tab_c = m->images + (m->precision == HTF_MLP_SPLIT ? Img<2>::TabC
                                      : m->precision == HTF_MLP_BF16 ? Img<1>::TabC
                                      : m->precision == HTF_MLP_SPLIT16 ? Img<3>::TabC : Img<0>::TabC);
    const float ginv = 1.0f / m->gap;
    const dim3 grid(nw / 4), block(256);
    dispatch_flags([&](auto TANH, auto F64) {
        using IT = scalar_t<F64>;
        hipLaunchKernelGGL((mlp_grad_kernel<TANH, IT>), grid, block, 0, stream, (const typename Vec4<IT>::type *)nlist, B, NN, labels, lab_f64,
                           predbuf, m->theta, dm, tab_c, ginv, partial, stride);
    }, th, in_dtype != HTF_F32);
    rc = check_launch("mlp_grad_kernel");
    if (rc != HTF_OK) return rc;
    hipLaunchKernelGGL(mlp_reduce_partials_kernel, dim3((ncols + 63) / 64), dim3(64 * kRedSlices), 0, stream, partial, nw, stride,
                       ncols, accum, (const float *)nullptr, 1);
    return check_launch("mlp_reduce_partials_kernel");
#else
    return HTF_OK; // (unreachable: force_valu is false in the shipped build)
#endif
}

} // namespace htf
