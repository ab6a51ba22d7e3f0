// Neighbor selection shared by the two neighbor-list searches of compute_nlist: the all-pairs kernel (cg_map.hip) and the
// cell-binned one (nlist_cells.hip).  Both translation units are built with -ffp-contract=off, so pair_of forms every
// distance as oracle.compute_nlist does -- fp32 differences, d - rint(d / L) * L, (x^2 + y^2) + z^2, correctly rounded
// sqrt -- and the two routes see the same bits for every pair.
//
// A row keeps its best NN candidates as sorted 64-bit keys in registers (slot s = k * 64 + lane, K = ceil(NN / 64) per lane):
//   high word: the distance's bits (sorted: nearest first) or their complement (unsorted: farthest first), low word: j,
// so "smaller key" is exactly the oracle's stable order and every key is distinct.  The list a row ends with is the NN
// smallest keys it was offered, whatever order they arrived in.
#pragma once

namespace htf_nlist {

constexpr unsigned long long kEmpty = ~0ull;

struct Pair {
    float x, y, z, d;
};

__device__ __forceinline__ float min_image(float d, float L) { return __fsub_rn(d, __fmul_rn(rintf(__fdiv_rn(d, L)), L)); }

__device__ __forceinline__ Pair pair_of(float xi, float yi, float zi, float xj, float yj, float zj, float Lx, float Ly, float Lz) {
    Pair p;
    p.x = min_image(__fsub_rn(xj, xi), Lx);
    p.y = min_image(__fsub_rn(yj, yi), Ly);
    p.z = min_image(__fsub_rn(zj, zi), Lz);
    p.d = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.y, p.y)), __fmul_rn(p.z, p.z)));
    return p;
}

// the key of pair (i, j), or kEmpty when the pair is out of range or excluded (excl: [M, M], applied both ways; nullable)
__device__ __forceinline__ unsigned long long key_of(const Pair &p, float r_cut, int sorted, const unsigned char *__restrict__ excl,
                                                     unsigned i, unsigned j, unsigned M) {
    bool ok = p.d <= r_cut && p.d >= 5e-4f;
    if (ok && excl) ok = !excl[(size_t)i * M + j] && !excl[(size_t)j * M + i];
    if (!ok) return kEmpty;
    const unsigned bits = __float_as_uint(p.d);
    return ((unsigned long long)(sorted ? bits : ~bits) << 32) | j;
}

// Offer every lane's candidate key to the wave's list: a candidate below the current worst key is inserted with one ballot
// (its rank) and one shift of the list by a lane.  worst: the key of slot NN - 1 (kEmpty until the list is full).
template <int K>
__device__ __forceinline__ void offer(unsigned long long (&key)[K], unsigned long long &worst, unsigned long long cand, unsigned lane,
                                      unsigned NN, unsigned last_k, unsigned last_lane) {
    unsigned long long pending = __ballot(cand < worst);
    while (pending) {
        const int src = __builtin_ctzll(pending);
        pending &= pending - 1ull;
        const unsigned long long nk = __shfl(cand, src);
        if (!(nk < worst)) continue; // (wave-uniform: the list moved since the ballot)
        unsigned rank = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) rank += (unsigned)__popcll(__ballot(key[k] < nk));
        // shift slots >= rank up by one, nk into slot rank; the highest slot k reads lane 63 of slot k - 1 (not yet moved)
#pragma unroll
        for (int k = K - 1; k >= 0; --k) {
            unsigned long long up = __shfl_up(key[k], 1u);
            const unsigned long long carry = k > 0 ? __shfl(key[k > 0 ? k - 1 : 0], 63) : kEmpty;
            if (lane == 0) up = carry;
            const unsigned s = (unsigned)k * 64u + lane;
            key[k] = s < rank ? key[k] : (s == rank ? nk : up);
            if (s >= NN) key[k] = kEmpty;
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            if ((unsigned)k == last_k) worst = __shfl(key[k], (int)last_lane);
    }
}

// Row i of the output: [NN, 4] = (minimum-image vector, neighbor index or type) and idx [NN] (-1 = empty slot), the vector
// formed again from the raw positions exactly as it was measured.
template <int K>
__device__ __forceinline__ void write_row(const unsigned long long (&key)[K], unsigned lane, unsigned i, unsigned NN, const float *__restrict__ pos,
                                          unsigned stride, float xi, float yi, float zi, float Lx, float Ly, float Lz, int return_types,
                                          float *__restrict__ out, int *__restrict__ out_idx) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned s = (unsigned)k * 64u + lane;
        if (s >= NN) continue;
        const size_t o = (size_t)i * NN + s;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        int jj = -1;
        if (key[k] != kEmpty) {
            const unsigned j = (unsigned)(key[k] & 0xffffffffull);
            const Pair p = pair_of(xi, yi, zi, pos[(size_t)j * stride + 0], pos[(size_t)j * stride + 1], pos[(size_t)j * stride + 2],
                                   Lx, Ly, Lz);
            v = make_float4(p.x, p.y, p.z, return_types ? pos[(size_t)j * stride + 3] : (float)j);
            jj = (int)j;
        }
        reinterpret_cast<float4 *>(out)[o] = v;
        out_idx[o] = jj;
    }
}

} // namespace htf_nlist
