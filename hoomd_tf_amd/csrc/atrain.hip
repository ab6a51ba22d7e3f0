// Force matching on the conservative forces of the descriptor network with angular channels (include/htf_atrain.h,
// htf.DescriptorMLP.angular_loss_gradient): d SSR / d theta for F = -d(sum_i E_i)/dr of an l_max = 1 or 2 layer in one sweep
// over the pair vectors.
//
// With the residual held fixed, rho . F is row by row the derivative of E_i along a tangent of its own input X = [G | A | Q]
// (DESIGN.md 0.7), so the row is dtrain_row.h's with another front: step 1 keeps, per live slot, the direction u, the
// projection a = d . u of d = rho_i - m rho_j and dperp / r; step 2 forms, per channel and from one exponential per slot, the
// fixed-order wave sums of w, w' a, w u, vdot and (l_max = 2) M, Mdot -- 8 or 20 of them -- and lane c < Dr turns its channel's
// into A, Adot, Q, Qdot and writes the three entries it owns of the two input lines.  Steps 3 to 5 -- forward with tangent,
// reverse, register accumulators, block partials -- are dtrain_rows' statement for statement over D = Dr (1 + l_max) inputs
// (called as functions shared with dtrain_rows they cost the l_max = 2 forms 0.9 %: HISTORY.md), the slots are read by
// desc_row.h's desc_slot, and the partials are added by bp.hip's dtrain_reduce_kernel, the library's one reduction.  Every term lands on the row that
// reads it: no atomics, no scatter.  Built with -ffp-contract=on like bp.o (csrc/Makefile).
#include "htf_atrain.h"
#include "htf_cghost.h"
#include "dtrain_row.h"

namespace htf {
namespace {

// n work items: rows 0 .. n - 1, or rows[0 .. n - 1] with LIST (rows is then not null); one partial [1 + P] per block
template <bool TANH, bool CUT, bool LIST, int LMAX, typename IT>
__device__ __forceinline__ void at_rows(const typename Vec4<IT>::type *__restrict__ nlist, const int *__restrict__ index,
                                        const int *__restrict__ rows, unsigned n, unsigned B, unsigned NN,
                                        const float *__restrict__ weights, const float *__restrict__ mu, int K, int T, int H1, int H2,
                                        float gap, float rc, const float4 *__restrict__ rho, float *__restrict__ partials) {
    extern __shared__ float s_mem[];
    const int Dr = K * T;
    const int D = Dr * (1 + LMAX);
    const int ld1 = H1 + 1, ld2 = H2 + 1;   // (odd row strides: dtrain_row.h)
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
        const float4 pr = rho[row];
        const float rx = pr.x, ry = pr.y, rz = pr.z, re = pr.w;
        assr += (rx * rx + ry * ry) + (rz * rz + re * re);

        // 1. this lane's slots: distance, type (-1: contributes nothing), direction u, a = d . u and dperp / r = (d - a u) / r
        //    of d = rho_i - rho_j (rho_i alone for j outside [0, B))
        const typename Vec4<IT>::type *rp = nlist + (size_t)row * NN;
        float r[kDescSlots], a[kDescSlots];
        float ux[kDescSlots], uy[kDescSlots], uz[kDescSlots];
        float px[kDescSlots], py[kDescSlots], pz[kDescSlots];
        float fc[kDescSlots], dfc[kDescSlots];   // (CUT only)
        int ty[kDescSlots];
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) {
            const unsigned slot = t * 64 + lane;
            r[t] = 1.f;
            a[t] = 0.f;
            ux[t] = uy[t] = uz[t] = 0.f;
            px[t] = py[t] = pz[t] = 0.f;
            fc[t] = dfc[t] = 0.f;
            ty[t] = -1;
            if ((unsigned)t < ns && slot < NN) {
                const DescSlot s = desc_slot<IT>(&rp[slot], T);
                bool live = s.rr > kRinvDelta && s.typ >= 0;
                if constexpr (CUT) live = live && s.rr < rc;
                if (live) {
                    r[t] = s.rr;
                    ty[t] = s.typ;
                    ux[t] = s.tx / s.rr; uy[t] = s.tyy / s.rr; uz[t] = s.tz / s.rr;
                    float dx = rx, dy = ry, dz = rz;
                    const int j = index[(size_t)row * NN + slot];
                    if ((unsigned)j < B) {   // (a negative index is above B as unsigned)
                        const float4 rj = rho[j];
                        dx -= rj.x; dy -= rj.y; dz -= rj.z;
                    }
                    const float aa = dx * ux[t] + dy * uy[t] + dz * uz[t];
                    a[t] = aa;
                    px[t] = (dx - aa * ux[t]) / s.rr; py[t] = (dy - aa * uy[t]) / s.rr; pz[t] = (dz - aa * uz[t]) / s.rr;
                    if constexpr (CUT) cutoff_terms(s.rr, rc, c_fc, fc[t], dfc[t]);
                }
            }
        }

        // 2. the moments and their tangents from the same exponentials: lane t*K + k ends up holding those of channel k of type t
        float G = 0.f, Gd = 0.f, vx = 0.f, vy = 0.f, vz = 0.f, wx = 0.f, wy = 0.f, wz = 0.f;
        float mxx = 0.f, mxy = 0.f, mxz = 0.f, myy = 0.f, myz = 0.f, mzz = 0.f;
        float nxx = 0.f, nxy = 0.f, nxz = 0.f, nyy = 0.f, nyz = 0.f, nzz = 0.f;
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
                float p = 0.f, pd = 0.f, sx = 0.f, sy = 0.f, sz = 0.f, tx = 0.f, tyy = 0.f, tz = 0.f;
                float qxx = 0.f, qxy = 0.f, qxz = 0.f, qyy = 0.f, qyz = 0.f, qzz = 0.f;
                float oxx = 0.f, oxy = 0.f, oxz = 0.f, oyy = 0.f, oyz = 0.f, ozz = 0.f;
#pragma unroll
                for (int t = 0; t < kDescSlots; ++t)
                    if ((unsigned)t < ns) {
                        const float w = ty[t] == tt ? e[t] : 0.f;
                        const float wd = ty[t] == tt ? ed[t] : 0.f;
                        p += w;
                        pd += wd;
                        const float wux = w * ux[t], wuy = w * uy[t], wuz = w * uz[t];
                        sx += wux; sy += wuy; sz += wuz;
                        const float dux = wd * ux[t], duy = wd * uy[t], duz = wd * uz[t];
                        tx += dux + w * px[t]; tyy += duy + w * py[t]; tz += duz + w * pz[t];
                        if constexpr (LMAX == 2) {
                            qxx += wux * ux[t]; qxy += wux * uy[t]; qxz += wux * uz[t];
                            qyy += wuy * uy[t]; qyz += wuy * uz[t]; qzz += wuz * uz[t];
                            oxx += dux * ux[t] + 2.0f * (wux * px[t]);
                            oxy += dux * uy[t] + (wux * py[t] + wuy * px[t]);
                            oxz += dux * uz[t] + (wux * pz[t] + wuz * px[t]);
                            oyy += duy * uy[t] + 2.0f * (wuy * py[t]);
                            oyz += duy * uz[t] + (wuy * pz[t] + wuz * py[t]);
                            ozz += duz * uz[t] + 2.0f * (wuz * pz[t]);
                        }
                    }
                const bool mine = (int)lane == tt * K + k;
                p = group_sum<64>(p); pd = group_sum<64>(pd);
                sx = group_sum<64>(sx); sy = group_sum<64>(sy); sz = group_sum<64>(sz);
                tx = group_sum<64>(tx); tyy = group_sum<64>(tyy); tz = group_sum<64>(tz);
                if (mine) { G = p; Gd = pd; vx = sx; vy = sy; vz = sz; wx = tx; wy = tyy; wz = tz; }
                if constexpr (LMAX == 2) {
                    qxx = group_sum<64>(qxx); qxy = group_sum<64>(qxy); qxz = group_sum<64>(qxz);
                    qyy = group_sum<64>(qyy); qyz = group_sum<64>(qyz); qzz = group_sum<64>(qzz);
                    oxx = group_sum<64>(oxx); oxy = group_sum<64>(oxy); oxz = group_sum<64>(oxz);
                    oyy = group_sum<64>(oyy); oyz = group_sum<64>(oyz); ozz = group_sum<64>(ozz);
                    if (mine) {
                        mxx = qxx; mxy = qxy; mxz = qxz; myy = qyy; myz = qyz; mzz = qzz;
                        nxx = oxx; nxy = oxy; nxz = oxz; nyy = oyy; nyz = oyz; nzz = ozz;
                    }
                }
            }
        }

        // the input lines [G | A | Q] and [Gdot | Adot | Qdot]: lane c < Dr writes its channel's entries, lanes past D their own
        // zero (every entry of a line has one writer)
        __builtin_amdgcn_wave_barrier();   // (the previous row's lines have been read by every lane)
        if ((int)lane < Dr) {
            sG[lane] = G;
            sGd[lane] = Gd;
            sG[Dr + lane] = vx * vx + vy * vy + vz * vz;
            sGd[Dr + lane] = 2.0f * (vx * wx + vy * wy + vz * wz);
            if constexpr (LMAX == 2) {
                sG[2 * Dr + lane] = (mxx * mxx + myy * myy + mzz * mzz) + 2.0f * (mxy * mxy + mxz * mxz + myz * myz);
                sGd[2 * Dr + lane] = 2.0f * ((mxx * nxx + myy * nyy + mzz * nzz) + 2.0f * (mxy * nxy + mxz * nxz + myz * nyz));
            }
        }
        if ((int)lane >= D) sG[lane] = sGd[lane] = 0.f;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();

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

template <bool TANH, bool CUT, bool LIST, int LMAX, typename IT>
__global__ __launch_bounds__(256, 1) void at_sweep_kernel(const typename Vec4<IT>::type *__restrict__ nlist, const int *__restrict__ index,
                                                          const int *__restrict__ rows, unsigned n, unsigned B, unsigned NN,
                                                          const float *__restrict__ weights, const float *__restrict__ mu, int K, int T,
                                                          int H1, int H2, float gap, float rc, const float4 *__restrict__ rho,
                                                          float *__restrict__ partials) {
    at_rows<TANH, CUT, LIST, LMAX, IT>(nlist, index, rows, n, B, NN, weights, mu, K, T, H1, H2, gap, rc, rho, partials);
}

int at_check(unsigned B, unsigned n_rows, unsigned K, unsigned T, unsigned l_max, float r_cut) {
    HTF_REQUIRE(l_max == 1 || l_max == 2, "descriptor network: l_max = %u; the angular sweep takes 1 or 2 (0: htf_ctrain.h)", l_max);
    HTF_REQUIRE(K * T * (1 + l_max) <= (unsigned)kDescMaxD, "descriptor network: K n_types (1 + l_max) = %u * %u * %u inputs; at most %d",
                K, T, 1 + l_max, kDescMaxD);
    return desc_check_rows(B, n_rows, r_cut);
}

} // namespace
} // namespace htf

// (the index bound of the sweep is the residual table's n_table rows; the row count stays n_rows of B)
extern "C" int htf_at_loss_grad_ghost(const void *d_nlist, int nlist_dtype, const int *d_index, unsigned B, unsigned NN, unsigned K,
                                      unsigned n_types, unsigned H1, unsigned H2, int activation, const float *d_weights,
                                      const float *d_mu, float gap, const float *d_rho, float *d_accum, float *d_scratch,
                                      const int *d_rows, unsigned n_rows, float r_cut, unsigned l_max, unsigned n_table,
                                      htf_stream stream) {
    using namespace htf;
    HTF_REQUIRE(n_table >= B, "descriptor network: n_table %u < B %u", n_table, B);
    // (the residual table stands where htf_bp_loss_grad has the labels and the prediction)
    int rc = dtrain_check_call(d_nlist, nlist_dtype, B, NN, K, n_types, H1, H2, activation, d_weights, d_mu, gap, d_rho, HTF_F32, d_rho,
                               d_accum, d_scratch);
    if (rc != HTF_OK) return rc;
    HTF_REQUIRE(B == 0 || d_index, "descriptor network: null pointer");
    if ((rc = at_check(B, n_rows, K, n_types, l_max, r_cut)) != HTF_OK) return rc;
    if (!d_accum) return HTF_OK;   // (B = 0 and nothing to zero-fill: no launch)
    const unsigned Tw = n_types * (1u + l_max);   // (the weights, the lines and the partials are those of K Tw inputs)
    const unsigned n = 1u + dtrain_params(K * Tw, H1, H2);
    const unsigned grid = dtrain_grid(n_rows);   // (0 for no rows: the reduction alone then writes zeros)
    const hipStream_t s = (hipStream_t)stream;
    if (grid) {
        const size_t lds = dtrain_lds(K, Tw, H1, H2);
        dispatch_flags([&](auto TANH, auto CUT, auto LIST, auto L2, auto F64) {
            using IT = scalar_t<F64>;
            hipLaunchKernelGGL((at_sweep_kernel<TANH, CUT, LIST, L2 ? 2 : 1, IT>), dim3(grid), dim3(256), lds, s,
                               (const typename Vec4<IT>::type *)d_nlist, d_index, d_rows, n_rows, n_table, NN, d_weights, d_mu, (int)K,
                               (int)n_types, (int)H1, (int)H2, gap, r_cut, (const float4 *)d_rho, d_scratch);
        }, activation == HTF_ACT_TANH, r_cut > 0.0f, d_rows != nullptr, l_max == 2, nlist_dtype == HTF_F64);
        const int rl = check_launch("at_sweep_kernel");
        if (rl != HTF_OK) return rl;
    }
    return dtrain_reduce_launch(d_scratch, grid, n, d_accum, s);
}

extern "C" int htf_at_loss_grad(const void *d_nlist, int nlist_dtype, const int *d_index, unsigned B, unsigned NN, unsigned K,
                                unsigned n_types, unsigned H1, unsigned H2, int activation, const float *d_weights, const float *d_mu,
                                float gap, const float *d_rho, float *d_accum, float *d_scratch, const int *d_rows, unsigned n_rows,
                                float r_cut, unsigned l_max, htf_stream stream) {
    return htf_at_loss_grad_ghost(d_nlist, nlist_dtype, d_index, B, NN, K, n_types, H1, H2, activation, d_weights, d_mu, gap, d_rho,
                                  d_accum, d_scratch, d_rows, n_rows, r_cut, l_max, B, stream);
}
