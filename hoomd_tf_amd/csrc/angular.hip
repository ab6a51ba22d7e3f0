// Angular channels of the descriptor network on its conservative forces (include/htf_angular.h,
// htf.DescriptorMLP(conservative=True, l_max=1 or 2)): the two sweeps of cforce.hip with neighbor moments.
//
// Pass 1 (ang_grad_kernel) is desc_row.h's row through step 4 with the moments in step 2: one wave per row, slots in
// registers with their direction u, and for every channel c = t K + k ten fixed-order wave sums at most -- G, the vector
// v = sum w u (l_max >= 1) and the symmetric tensor M = sum w u (outer) u (l_max = 2) -- kept by lane c.  Lane c forms
// A = |v|^2 and Q = ||M||_F^2, the wave publishes [G | A | Q] (D = Dr (1 + l_max) values) to its exchange line, and the network
// runs forward and backward over D lanes exactly as in desc_row.h.  Lane c < Dr then reads its two other derivatives from the
// line and writes its C = 4 or 10 floats {g, p = 2 g_A v, S = 2 g_Q M} to the table h [B][Dr][C]; lane 0 writes E_i.
// ang_desc_kernel is the same row ending after the moments: the bits pass 1 feeds the network.
//
// Pass 2 (ang_force_kernel) is cf_pair_force_kernel with the table in place of g: the wave stages its own Dr C floats in a
// wave-private LDS region (at most 210 floats), each lane gathers the contiguous K C floats h[j][t_i K ..] of its slots -- a
// float4 per channel for C = 4, five float2 for C = 10 (the table is 16-byte aligned, so those are always aligned) --
// recomputes the exponentials, and contracts the gathered terms with the slot's own u as they arrive: five accumulators per
// slot (six with a cutoff), a coefficient along u and a 3-vector.  F_i and the nine entries of W_i follow by the fixed-order
// wave sums of desc_pair_force_end (desc_row.h), cf_pair_force_kernel's own end.  No atomics, no scratch; built with -ffp-contract=on like bp.o (csrc/Makefile), so that both instantiations
// of the row form the moments alike.
#include "htf_angular.h"
#include "htf_cghost.h"
#include "desc_row.h"

namespace htf {
namespace {

constexpr int kAngRegion = 212;   // floats of a wave's own table row in LDS: Dr C <= 32 * 4, 21 * 10 = 210

__host__ __device__ constexpr int ang_width(int lmax) { return lmax == 1 ? 4 : 10; }

// NET = false: the network input alone, out [B][D].  NET = true: table [B][Dr][C] and energy [B].
// n work items: rows 0 .. n - 1, or rows[0 .. n - 1] when rows is not null (wave-uniform).
template <bool NET, bool TANH, bool CUT, int LMAX, typename IT>
__device__ __forceinline__ void ang_rows(const typename Vec4<IT>::type *__restrict__ nlist, const int *__restrict__ rows, unsigned n,
                                         unsigned NN, const float *__restrict__ weights, const float *__restrict__ mu, int K, int T,
                                         int H1, int H2, float gap, float rc, float *__restrict__ table, float *__restrict__ energy_out,
                                         void *__restrict__ out, int out_f64) {
    extern __shared__ float s_mem[];
    constexpr int C = ang_width(LMAX);
    const int Dr = K * T;
    const int D = Dr * (1 + LMAX);
    const int ld1 = H1 + 1, ld2 = H2 + 1;   // (odd row strides: desc_row.h)
    const int nw = NET ? desc_lds_weights(D, H1, H2) : 0;
    float *s_w = s_mem;
    float *s_mu = s_w + ((nw + 3) & ~3);
    float *s_x = s_mu + ((K + 3) & ~3) + (threadIdx.x >> 6) * 64; // this wave's exchange line
    float *W1 = s_w, *b1 = W1 + D * ld1, *W2 = b1 + H1, *b2 = W2 + H1 * ld2, *W3 = b2 + H2, *b3 = W3 + H2;
    if constexpr (NET) {
        const float *g_b1 = weights + D * H1, *g_W2 = g_b1 + H1, *g_b2 = g_W2 + H1 * H2;
        for (int i = threadIdx.x; i < D * H1; i += blockDim.x) W1[(i / H1) * ld1 + i % H1] = weights[i];
        for (int i = threadIdx.x; i < H1 * H2; i += blockDim.x) W2[(i / H2) * ld2 + i % H2] = g_W2[i];
        for (int i = threadIdx.x; i < H1; i += blockDim.x) b1[i] = g_b1[i];
        for (int i = threadIdx.x; i < 2 * H2 + 1; i += blockDim.x) b2[i] = g_b2[i]; // b2 | W3 | b3, contiguous in both
    }
    for (int i = threadIdx.x; i < K; i += blockDim.x) s_mu[i] = mu[i];
    __syncthreads();

    const float c_exp = -1.4426950408889634f / gap; // exp(-d^2 / gap) = exp2(c_exp d^2)
    const float c_fc = CUT ? cutoff_slope(rc) : 0.f;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned ns = (NN + 63u) >> 6;            // slots per lane in use (wave-uniform)
    const unsigned stride = gridDim.x * (blockDim.x >> 6);

    for (unsigned q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); q < n; q += stride) { // wave-uniform
        const unsigned row = rows ? (unsigned)rows[q] : q;
        const typename Vec4<IT>::type *rp = nlist + (size_t)row * NN;

        // 1. this lane's slots, by the arithmetic of desc_row.h's desc_slot and step 1 (written out: through desc_slot the
        //    l_max = 2 forms took 8 fewer VGPRs and total_forces 0.3 % longer), and their direction u = (x + 1e-7) / r
        float ux[kDescSlots], uy[kDescSlots], uz[kDescSlots], r[kDescSlots], fc[kDescSlots];
        int ty[kDescSlots];
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) {
            const unsigned slot = t * 64 + lane;
            ux[t] = uy[t] = uz[t] = 0.f;
            r[t] = 1.f;
            fc[t] = 0.f;
            ty[t] = -1;
            if ((unsigned)t < ns && slot < NN) {
                const auto v = load_stream(&rp[slot]);
                const float tx = (float)v.x + kNormDelta, tyy = (float)v.y + kNormDelta, tz = (float)v.z + kNormDelta;
                const float rr = sqrtf(tx * tx + tyy * tyy + tz * tz);
                int typ = 0;
                if (T > 1) {
                    const IT rw = rint(v.w);
                    typ = (rw >= (IT)0 && rw < (IT)T) ? (int)rw : -1; // (NaN: -1)
                }
                bool live = rr > kRinvDelta && typ >= 0;
                if constexpr (CUT) live = live && rr < rc;
                if (live) {
                    r[t] = rr;
                    ty[t] = typ;
                    ux[t] = tx / rr; uy[t] = tyy / rr; uz[t] = tz / rr;
                    if constexpr (CUT) {
                        float dfc;
                        cutoff_terms(rr, rc, c_fc, fc[t], dfc);
                    }
                }
            }
        }

        // 2. the moments: lane t*K + k ends up holding G, v and M of channel k of type t
        float G = 0.f, vx = 0.f, vy = 0.f, vz = 0.f;
        float mxx = 0.f, mxy = 0.f, mxz = 0.f, myy = 0.f, myz = 0.f, mzz = 0.f;
        for (int k = 0; k < K; ++k) {
            const float m = s_mu[k];
            float e[kDescSlots];
#pragma unroll
            for (int t = 0; t < kDescSlots; ++t) e[t] = 0.f;
#pragma unroll
            for (int t = 0; t < kDescSlots; ++t) {
                if ((unsigned)t >= ns) break;   // (a break keeps the wave-uniform branch: desc_row.h)
                const float d = r[t] - m;
                const float ev = __builtin_amdgcn_exp2f(c_exp * (d * d));
                if constexpr (CUT)
                    e[t] = ty[t] >= 0 ? fc[t] * ev : 0.f;
                else
                    e[t] = ty[t] >= 0 ? ev : 0.f;
            }
            for (int tt = 0; tt < T; ++tt) {
                float p = 0.f, px = 0.f, py = 0.f, pz = 0.f;
                float qxx = 0.f, qxy = 0.f, qxz = 0.f, qyy = 0.f, qyz = 0.f, qzz = 0.f;
#pragma unroll
                for (int t = 0; t < kDescSlots; ++t) {
                    if ((unsigned)t < ns) {
                        const float w = ty[t] == tt ? e[t] : 0.f;
                        p += w;
                        const float wx = w * ux[t], wy = w * uy[t], wz = w * uz[t];
                        px += wx; py += wy; pz += wz;
                        if constexpr (LMAX == 2) {
                            qxx += wx * ux[t]; qxy += wx * uy[t]; qxz += wx * uz[t];
                            qyy += wy * uy[t]; qyz += wy * uz[t]; qzz += wz * uz[t];
                        }
                    }
                }
                const bool mine = (int)lane == tt * K + k;
                p = group_sum<64>(p);
                px = group_sum<64>(px); py = group_sum<64>(py); pz = group_sum<64>(pz);
                if (mine) { G = p; vx = px; vy = py; vz = pz; }
                if constexpr (LMAX == 2) {
                    qxx = group_sum<64>(qxx); qxy = group_sum<64>(qxy); qxz = group_sum<64>(qxz);
                    qyy = group_sum<64>(qyy); qyz = group_sum<64>(qyz); qzz = group_sum<64>(qzz);
                    if (mine) { mxx = qxx; mxy = qxy; mxz = qxz; myy = qyy; myz = qyz; mzz = qzz; }
                }
            }
        }
        const float A = vx * vx + vy * vy + vz * vz;
        float Q = 0.f;
        if constexpr (LMAX == 2) Q = (mxx * mxx + myy * myy + mzz * mzz) + 2.0f * (mxy * mxy + mxz * mxz + myz * myz);
        if constexpr (!NET) {
            if ((int)lane < Dr) {
                const size_t o = (size_t)row * D + lane;
                if (out_f64) {
                    ((double *)out)[o] = G;
                    ((double *)out)[o + Dr] = A;
                    if constexpr (LMAX == 2) ((double *)out)[o + 2 * Dr] = Q;
                } else {
                    ((float *)out)[o] = G;
                    ((float *)out)[o + Dr] = A;
                    if constexpr (LMAX == 2) ((float *)out)[o + 2 * Dr] = Q;
                }
            }
            continue;
        }

        // 3. forward on [G | A | Q]: one hidden unit per lane (desc_row.h's step 3 over D inputs)
        __builtin_amdgcn_wave_barrier();   // (the previous row's line has been read by every lane)
        if ((int)lane < Dr) {
            s_x[lane] = G;
            s_x[Dr + lane] = A;
            if constexpr (LMAX == 2) s_x[2 * Dr + lane] = Q;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
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

        // 4. backward to g = dE/d(input), lane c < D
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
        line_publish(s_x, lane, gG);

        // 5. the table: lane c < Dr holds G's derivative and reads those of its A and Q from the line
        if ((int)lane < Dr) {
            const float pa = 2.0f * s_x[Dr + lane];
            float *hp = table + ((size_t)row * Dr + lane) * C;
            if constexpr (LMAX == 1) {
                *reinterpret_cast<float4 *>(hp) = make_float4(gG, pa * vx, pa * vy, pa * vz);
            } else {
                const float sa = 2.0f * s_x[2 * Dr + lane];
                float2 *h2p = reinterpret_cast<float2 *>(hp);   // (40-byte records: 8-byte aligned)
                h2p[0] = make_float2(gG, pa * vx);
                h2p[1] = make_float2(pa * vy, pa * vz);
                h2p[2] = make_float2(sa * mxx, sa * mxy);
                h2p[3] = make_float2(sa * mxz, sa * myy);
                h2p[4] = make_float2(sa * myz, sa * mzz);
            }
        }
        if (lane == 0) energy_out[row] = energy;
    }
}

template <bool TANH, bool CUT, int LMAX, typename IT>
__global__ __launch_bounds__(256) void ang_grad_kernel(const typename Vec4<IT>::type *__restrict__ nlist, const int *__restrict__ rows,
                                                       unsigned n, unsigned NN, const float *__restrict__ weights,
                                                       const float *__restrict__ mu, int K, int T, int H1, int H2, float gap, float rc,
                                                       float *__restrict__ table, float *__restrict__ energy) {
    ang_rows<true, TANH, CUT, LMAX, IT>(nlist, rows, n, NN, weights, mu, K, T, H1, H2, gap, rc, table, energy, nullptr, 0);
}

template <bool CUT, int LMAX, typename IT>
__global__ __launch_bounds__(256) void ang_desc_kernel(const typename Vec4<IT>::type *__restrict__ nlist, unsigned n, unsigned NN,
                                                       const float *__restrict__ mu, int K, int T, float gap, float rc,
                                                       void *__restrict__ out, int out_f64) {
    ang_rows<false, false, CUT, LMAX, IT>(nlist, nullptr, n, NN, nullptr, mu, K, T, 0, 0, gap, rc, nullptr, nullptr, out, out_f64);
}

// n_table >= B: the rows of the table (include/htf_cghost.h); rows [B, n_table) are ghosts' rows, read through a slot's index only
template <bool VIRIAL, bool CUT, int LMAX, typename IT>
__global__ __launch_bounds__(256) void ang_force_kernel(const typename Vec4<IT>::type *__restrict__ nlist, const int *__restrict__ index,
                                                        const float *__restrict__ types, unsigned B, unsigned n_table, unsigned NN,
                                                        const float *__restrict__ mu, int K, int T, float gap, float rc,
                                                        const float *__restrict__ table, const float *__restrict__ energy,
                                                        void *__restrict__ out, int out_f64, void *__restrict__ virial9) {
    extern __shared__ float s_mem[];
    constexpr int C = ang_width(LMAX);
    const int Dr = K * T;
    const int rowlen = Dr * C;                                        // <= 210 <= kAngRegion
    float *s_mu = s_mem;
    float *s_h = s_mu + ((K + 3) & ~3) + (threadIdx.x >> 6) * kAngRegion; // this wave's own table row
    for (int i = threadIdx.x; i < K; i += blockDim.x) s_mu[i] = mu[i];
    __syncthreads();

    const float c_exp = -1.4426950408889634f / gap; // exp(-d^2 / gap) = exp2(c_exp d^2)
    const float c_der = -2.0f / gap;                // d e / d r = c_der (r - mu) e
    const float c_fc = CUT ? cutoff_slope(rc) : 0.f;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned ns = (NN + 63u) >> 6;            // slots per lane in use (wave-uniform)
    const unsigned stride = gridDim.x * (blockDim.x >> 6);
    // the index bound in a vector register: as one more scalar held across the row loop it spilled two SGPRs in three forms
    unsigned n_index = n_table;
    asm volatile("" : "+v"(n_index));

    for (unsigned row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); row < B; row += stride) { // wave-uniform
        const typename Vec4<IT>::type *rp = nlist + (size_t)row * NN;
        const int *ip = index + (size_t)row * NN;

        // 1. this lane's slots as cf_pair_force_kernel keeps them (near on the distance alone, ty = -1 empties the own-row terms)
        float x[kDescSlots], y[kDescSlots], z[kDescSlots], r[kDescSlots];
        float ux[kDescSlots], uy[kDescSlots], uz[kDescSlots];
        float fc[kDescSlots], dfc[kDescSlots];   // (CUT only)
        int ty[kDescSlots];
        bool near[kDescSlots];
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) {
            const unsigned slot = t * 64 + lane;
            x[t] = y[t] = z[t] = 0.f;
            ux[t] = uy[t] = uz[t] = 0.f;
            r[t] = 1.f;
            fc[t] = dfc[t] = 0.f;
            ty[t] = -1;
            near[t] = false;
            if ((unsigned)t < ns && slot < NN) {
                const DescSlot s = desc_slot<IT>(&rp[slot], T);
                x[t] = s.x; y[t] = s.y; z[t] = s.z;
                bool live = s.rr > kRinvDelta;
                if constexpr (CUT) live = live && s.rr < rc;
                if (live) {
                    near[t] = true;
                    r[t] = s.rr;
                    ty[t] = s.typ;
                    ux[t] = s.tx / s.rr; uy[t] = s.tyy / s.rr; uz[t] = s.tz / s.rr;
                    if constexpr (CUT) cutoff_terms(s.rr, rc, c_fc, fc[t], dfc[t]);
                }
            }
        }

        // 2. where each slot's reverse terms live: h[j][t_i K ..], or nowhere (index outside [0, n_table), own type out of range)
        int ti = 0;
        if (T > 1) {
            const float tw = rintf(types[row]);
            ti = (tw >= 0.f && tw < (float)T) ? (int)tw : -1; // (NaN: -1)
        }
        const float *hj[kDescSlots];
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) {
            hj[t] = nullptr;
            if ((unsigned)t < ns && near[t] && ti >= 0) {   // (a kept slot: t * 64 + lane < NN)
                const int j = ip[t * 64 + lane];
                if ((unsigned)j < n_index) hj[t] = table + ((size_t)j * Dr + ti * K) * C;
            }
        }
        __builtin_amdgcn_wave_barrier();   // (the previous row's region has been read by every lane)
        for (int i = lane; i < rowlen; i += 64) s_h[i] = table[(size_t)row * rowlen + i];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();

        // 3. per slot, over k: X = s0 + dp.u + u.sS u and Y = dp + 2 sS u, accumulated against e_k (and X against d_k e_k)
        float aA[kDescSlots], aB[kDescSlots], aYx[kDescSlots], aYy[kDescSlots], aYz[kDescSlots];
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) aA[t] = aB[t] = aYx[t] = aYy[t] = aYz[t] = 0.f;
        for (int k = 0; k < K; ++k) {
            const float m = s_mu[k];
#pragma unroll
            for (int t = 0; t < kDescSlots; ++t) {
                if ((unsigned)t < ns) {
                    float hr[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) hr[c] = 0.f;
                    if (hj[t] != nullptr) {
                        if constexpr (LMAX == 1) {
                            const float4 v = *reinterpret_cast<const float4 *>(hj[t] + k * 4);
                            hr[0] = v.x; hr[1] = v.y; hr[2] = v.z; hr[3] = v.w;
                        } else {
                            const float2 *p2 = reinterpret_cast<const float2 *>(hj[t] + k * 10);
#pragma unroll
                            for (int c = 0; c < 5; ++c) {
                                const float2 v = p2[c];
                                hr[2 * c] = v.x; hr[2 * c + 1] = v.y;
                            }
                        }
                    }
                    const float *own = s_h + ((ty[t] > 0 ? ty[t] : 0) * K + k) * C;
                    float ho[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) ho[c] = ty[t] >= 0 ? own[c] : 0.f;
                    const float s0 = ho[0] + hr[0];
                    const float dpx = ho[1] - hr[1], dpy = ho[2] - hr[2], dpz = ho[3] - hr[3];
                    float X = s0 + (dpx * ux[t] + dpy * uy[t] + dpz * uz[t]);
                    float Yx = dpx, Yy = dpy, Yz = dpz;
                    if constexpr (LMAX == 2) {
                        const float sxx = ho[4] + hr[4], sxy = ho[5] + hr[5], sxz = ho[6] + hr[6];
                        const float syy = ho[7] + hr[7], syz = ho[8] + hr[8], szz = ho[9] + hr[9];
                        const float sux = sxx * ux[t] + sxy * uy[t] + sxz * uz[t];
                        const float suy = sxy * ux[t] + syy * uy[t] + syz * uz[t];
                        const float suz = sxz * ux[t] + syz * uy[t] + szz * uz[t];
                        X += sux * ux[t] + suy * uy[t] + suz * uz[t];
                        Yx += 2.0f * sux; Yy += 2.0f * suy; Yz += 2.0f * suz;
                    }
                    const float d = r[t] - m;
                    const float ev = __builtin_amdgcn_exp2f(c_exp * (d * d));
                    aA[t] = fmaf(X * d, ev, aA[t]);
                    if constexpr (CUT) aB[t] = fmaf(X, ev, aB[t]);
                    aYx[t] = fmaf(Yx, ev, aYx[t]);
                    aYy[t] = fmaf(Yy, ev, aYy[t]);
                    aYz[t] = fmaf(Yz, ev, aYz[t]);
                }
            }
        }

        // 4. phi = a u + b (no longer along x), F and W
        float fx = 0.f, fy = 0.f, fz = 0.f;
        float w[9];
#pragma unroll
        for (int c9 = 0; c9 < 9; ++c9) w[c9] = 0.f;
#pragma unroll
        for (int t = 0; t < kDescSlots; ++t) {
            if ((unsigned)t < ns && near[t]) {
                const float ir = 1.0f / r[t];
                const float yu = aYx[t] * ux[t] + aYy[t] * uy[t] + aYz[t] * uz[t];
                float a, b;
                if constexpr (CUT) {
                    b = fc[t] * ir;
                    a = fc[t] * (c_der * aA[t]) + dfc[t] * aB[t] - b * yu;
                } else {
                    b = ir;
                    a = c_der * aA[t] - b * yu;
                }
                const float ax = a * ux[t] + b * aYx[t], ay = a * uy[t] + b * aYy[t], az = a * uz[t] + b * aYz[t];
                fx += ax; fy += ay; fz += az;
                if constexpr (VIRIAL) {
                    const float hx = -0.5f * x[t], hy = -0.5f * y[t], hz = -0.5f * z[t];
                    w[0] += hx * ax; w[1] += hx * ay; w[2] += hx * az;
                    w[3] += hy * ax; w[4] += hy * ay; w[5] += hy * az;
                    w[6] += hz * ax; w[7] += hz * ay; w[8] += hz * az;
                }
            }
        }
        desc_pair_force_end<VIRIAL>(lane, row, fx, fy, fz, w, energy, out, out_f64, virial9);
    }
}

int ang_check(unsigned B, unsigned n_rows, unsigned K, unsigned T, unsigned l_max, float r_cut) {
    HTF_REQUIRE(l_max == 1 || l_max == 2, "descriptor network: l_max = %u; the angular entries take 1 or 2 (0: htf_cforce.h)", l_max);
    HTF_REQUIRE(K * T * (1 + l_max) <= (unsigned)kDescMaxD, "descriptor network: K n_types (1 + l_max) = %u * %u * %u inputs; at most %d",
                K, T, 1 + l_max, kDescMaxD);
    return desc_check_rows(B, n_rows, r_cut);
}

size_t ang_lds_forces(unsigned K) { return (((K + 3) & ~3u) + 4 * kAngRegion) * sizeof(float); }

} // namespace
} // namespace htf

extern "C" int htf_ang_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types, unsigned H1,
                            unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap, float *d_table,
                            float *d_energy, const int *d_rows, unsigned n_rows, float r_cut, unsigned l_max, htf_stream stream) {
    using namespace htf;
    int rc = desc_check(d_nlist, nlist_dtype, B, NN, K, n_types, d_mu, gap, d_table, HTF_F32);
    if (rc != HTF_OK) return rc;
    if ((rc = desc_check_network(d_weights, H1, H2, activation)) != HTF_OK) return rc;
    if ((rc = ang_check(B, n_rows, K, n_types, l_max, r_cut)) != HTF_OK) return rc;
    HTF_REQUIRE(B == 0 || d_energy, "descriptor network: null pointer");
    HTF_REQUIRE(((uintptr_t)d_table & 15u) == 0, "descriptor network: the table must be 16-byte aligned");
    if (n_rows == 0) return HTF_OK;
    const size_t lds = desc_lds_forces(K, n_types * (1 + l_max), H1, H2);   // (the weights of D = K n_types (1 + l_max) inputs)
    const hipStream_t s = (hipStream_t)stream;
    dispatch_flags([&](auto TANH, auto CUT, auto L2, auto F64) {
        using IT = scalar_t<F64>;
        hipLaunchKernelGGL((ang_grad_kernel<TANH, CUT, L2 ? 2 : 1, IT>), dim3(desc_grid(n_rows)), dim3(256), lds, s,
                           (const typename Vec4<IT>::type *)d_nlist, d_rows, n_rows, NN, d_weights, d_mu, (int)K, (int)n_types, (int)H1,
                           (int)H2, gap, r_cut, d_table, d_energy);
    }, activation == HTF_ACT_TANH, r_cut > 0.0f, l_max == 2, nlist_dtype == HTF_F64);
    return check_launch("ang_grad_kernel");
}

extern "C" int htf_ang_forces_ghost(const void *d_nlist, int nlist_dtype, const int *d_index, const float *d_types, unsigned B,
                                    unsigned NN, unsigned K, unsigned n_types, const float *d_mu, float gap, const float *d_table,
                                    const float *d_energy, void *d_force, int force_dtype, void *d_virial9, float r_cut,
                                    unsigned l_max, unsigned n_table, htf_stream stream) {
    using namespace htf;
    HTF_REQUIRE(n_table >= B, "descriptor network: n_table %u < B %u", n_table, B);
    int rc = desc_check(d_nlist, nlist_dtype, B, NN, K, n_types, d_mu, gap, d_force, force_dtype);
    if (rc != HTF_OK) return rc;
    if ((rc = ang_check(B, B, K, n_types, l_max, r_cut)) != HTF_OK) return rc;
    HTF_REQUIRE(B == 0 || (d_index && d_table && d_energy), "descriptor network: null pointer");
    HTF_REQUIRE(B == 0 || n_types == 1 || d_types, "descriptor network: n_types = %u needs the rows' own types", n_types);
    HTF_REQUIRE(((uintptr_t)d_table & 15u) == 0, "descriptor network: the table must be 16-byte aligned");
    if (B == 0) return HTF_OK;
    const size_t lds = ang_lds_forces(K);
    const int out_f64 = force_dtype == HTF_F64;
    const hipStream_t s = (hipStream_t)stream;
    dispatch_flags([&](auto VIR, auto CUT, auto L2, auto F64) {
        using IT = scalar_t<F64>;
        hipLaunchKernelGGL((ang_force_kernel<VIR, CUT, L2 ? 2 : 1, IT>), dim3(desc_grid(B)), dim3(256), lds, s,
                           (const typename Vec4<IT>::type *)d_nlist, d_index, d_types, B, n_table, NN, d_mu, (int)K, (int)n_types, gap,
                           r_cut, d_table, d_energy, d_force, out_f64, d_virial9);
    }, d_virial9 != nullptr, r_cut > 0.0f, l_max == 2, nlist_dtype == HTF_F64);
    return check_launch("ang_force_kernel");
}

// (the table is the pair tensor's own rows)
extern "C" int htf_ang_forces(const void *d_nlist, int nlist_dtype, const int *d_index, const float *d_types, unsigned B, unsigned NN,
                              unsigned K, unsigned n_types, const float *d_mu, float gap, const float *d_table, const float *d_energy,
                              void *d_force, int force_dtype, void *d_virial9, float r_cut, unsigned l_max, htf_stream stream) {
    return htf_ang_forces_ghost(d_nlist, nlist_dtype, d_index, d_types, B, NN, K, n_types, d_mu, gap, d_table, d_energy, d_force,
                                force_dtype, d_virial9, r_cut, l_max, B, stream);
}

extern "C" int htf_ang_descriptor(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types,
                                  const float *d_mu, float gap, void *d_out, int out_dtype, float r_cut, unsigned l_max,
                                  htf_stream stream) {
    using namespace htf;
    int rc = desc_check(d_nlist, nlist_dtype, B, NN, K, n_types, d_mu, gap, d_out, out_dtype);
    if (rc != HTF_OK) return rc;
    if ((rc = ang_check(B, B, K, n_types, l_max, r_cut)) != HTF_OK) return rc;
    if (B == 0) return HTF_OK;
    const size_t lds = desc_lds_descriptor(K);
    const int out_f64 = out_dtype == HTF_F64;
    const hipStream_t s = (hipStream_t)stream;
    dispatch_flags([&](auto CUT, auto L2, auto F64) {
        using IT = scalar_t<F64>;
        hipLaunchKernelGGL((ang_desc_kernel<CUT, L2 ? 2 : 1, IT>), dim3(desc_grid(B)), dim3(256), lds, s,
                           (const typename Vec4<IT>::type *)d_nlist, B, NN, d_mu, (int)K, (int)n_types, gap, r_cut, d_out, out_f64);
    }, r_cut > 0.0f, l_max == 2, nlist_dtype == HTF_F64);
    return check_launch("ang_desc_kernel");
}
