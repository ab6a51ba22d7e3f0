// Molecular geometry ops (include/htf_geom.h): bond lengths, bond angles and dihedrals of T terms, forward and backward.
//
// One lane per term, templated on the point count K.  The points come either from a molecule's rows (molecule mode: row
// t*MN + slot, the K slots by value) or from an int32 [T, K] table (CG mode).  The backward recomputes the geometry from
// the positions.  In molecule mode a term owns its molecule's rows, so the lane writes that block outright.  In CG mode a
// row can sit in many terms: the terms store their K contribution rows, then one lane per row sums its contribution rows
// in a fixed order through the inverted index (no atomics, bitwise reproducible).
#include "htf_common.h"
#include "htf_geom.h"

namespace {

struct V3 {
    float x, y, z;
};

__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator-(V3 a) { return {-a.x, -a.y, -a.z}; }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

__device__ __forceinline__ float min_image(float d, float L) { return d - rintf(d / L) * L; }

// the minimum image of q - p
__device__ __forceinline__ V3 wrapped(V3 q, V3 p, V3 L) {
    return {min_image(q.x - p.x, L.x), min_image(q.y - p.y, L.y), min_image(q.z - p.z, L.z)};
}

struct Slots {
    int s[4];
};

// row of point k of term t
template <int K, bool kTable>
__device__ __forceinline__ size_t point_row(unsigned t, int k, unsigned MN, const Slots &sl, const int *__restrict__ table) {
    if constexpr (kTable)
        return (size_t)table[(size_t)t * K + k];
    else
        return (size_t)t * MN + (size_t)sl.s[k];
}

template <int K, bool kTable>
__device__ __forceinline__ void load_points(V3 (&p)[K], const float *__restrict__ pos, unsigned stride, unsigned t, unsigned MN,
                                            const Slots &sl, const int *__restrict__ table) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float *q = pos + point_row<K, kTable>(t, k, MN, sl, table) * stride;
        p[k] = {q[0], q[1], q[2]};
    }
}

// The term's value and, with kGrad, g times its gradient with respect to each point in G.
template <int K, bool kGrad>
__device__ __forceinline__ float term(const V3 (&p)[K], V3 L, float g, V3 (&G)[K]) {
    if constexpr (K == 2) {
        const V3 d = wrapped(p[1], p[0], L);
        const float r = sqrtf(dot(d, d));
        if constexpr (kGrad) {
            G[1] = d * (r > 0.f ? g / r : 0.f);
            G[0] = -G[1];
        }
        return r;
    } else if constexpr (K == 3) {
        const V3 a = wrapped(p[0], p[1], L), b = wrapped(p[2], p[1], L);
        const V3 c = cross(a, b);
        const float s = sqrtf(dot(c, c));
        if constexpr (kGrad) {
            // d theta / d a = (a x c) / (|a|^2 s), d theta / d b = -(b x c) / (|b|^2 s): the components perpendicular to
            // the other vector, of length 1/|a| and 1/|b|; formed from c, so they stay accurate near 0 and pi
            const float da = dot(a, a) * s, db = dot(b, b) * s;
            G[0] = cross(a, c) * (da > 0.f ? g / da : 0.f);
            G[2] = cross(b, c) * (db > 0.f ? -g / db : 0.f);
            G[1] = -(G[0] + G[2]);
        }
        return atan2f(s, dot(a, b));
    } else {
        const V3 b1 = wrapped(p[1], p[0], L), b2 = wrapped(p[2], p[1], L), b3 = wrapped(p[3], p[2], L);
        const V3 n1 = cross(b1, b2), n2 = cross(b2, b3);
        const float n1s = dot(n1, n1), n2s = dot(n2, n2);
        const bool ok = n1s > 0.f && n2s > 0.f;
        const float gl2 = dot(b2, b2), gl = sqrtf(gl2);
        const float phi = ok ? atan2f(gl * dot(b1, n2), dot(n1, n2)) : 0.f;
        if constexpr (kGrad) {
            // Blondel & Karplus (J. Comput. Chem. 17, 1132, 1996) with F = -b1, G = -b2, H = b3, A = n1, B = n2, times
            // sign(phi): the op returns |phi|.  A degenerate term (n1 = 0 or n2 = 0) has sg = 0: a zero gradient.
            const bool gok = ok && gl2 > 0.f;
            const float sg = gok ? (phi > 0.f ? g : (phi < 0.f ? -g : 0.f)) : 0.f;
            const V3 ua = n1 * (gok ? sg * gl / n1s : 0.f), ub = n2 * (gok ? sg * gl / n2s : 0.f);
            const float inv = gok ? 1.f / gl2 : 0.f;
            const float fg = dot(b1, b2) * inv, hg = dot(b3, b2) * inv;
            G[0] = -ua;
            G[3] = ub;
            G[1] = ua + ua * fg + ub * hg;
            G[2] = -(ub + ua * fg + ub * hg);
        }
        return fabsf(phi);
    }
}

template <int K, bool kTable>
__global__ __launch_bounds__(256) void geom_forward_kernel(const float *__restrict__ pos, unsigned stride, unsigned T, unsigned MN,
                                                           Slots sl, const int *__restrict__ table,
                                                           const float *__restrict__ box_L, float *__restrict__ out) {
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const V3 L = {box_L[0], box_L[1], box_L[2]};
    V3 p[K], G[K];
    load_points<K, kTable>(p, pos, stride, t, MN, sl, table);
    out[t] = term<K, false>(p, L, 0.f, G);
}

// molecule mode: lane t writes all MN rows of molecule t (its K term rows, zeros elsewhere)
template <int K>
__global__ __launch_bounds__(256) void geom_mol_backward_kernel(const float *__restrict__ pos, unsigned stride, unsigned M,
                                                                unsigned MN, Slots sl, const float *__restrict__ box_L,
                                                                const float *__restrict__ gout, unsigned gstride,
                                                                float *__restrict__ gpos) {
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M) return;
    const V3 L = {box_L[0], box_L[1], box_L[2]};
    V3 p[K], G[K];
    load_points<K, false>(p, pos, stride, t, MN, sl, nullptr);
    term<K, true>(p, L, gout[(size_t)t * gstride], G);
    float *blk = gpos + (size_t)t * MN * 3;
    for (unsigned r = 0; r < MN; ++r) {
        V3 v = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < K; ++k)
            if ((int)r == sl.s[k]) v = G[k];
        blk[r * 3 + 0] = v.x;
        blk[r * 3 + 1] = v.y;
        blk[r * 3 + 2] = v.z;
    }
}

// CG mode, pass 1: term t stores the gradient of its point s as contribution row t*K + s
template <int K>
__global__ __launch_bounds__(256) void geom_cg_contrib_kernel(const float *__restrict__ pos, unsigned stride, unsigned T,
                                                              const int *__restrict__ table, const float *__restrict__ box_L,
                                                              const float *__restrict__ gout, unsigned gstride,
                                                              float *__restrict__ contrib) {
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const V3 L = {box_L[0], box_L[1], box_L[2]};
    V3 p[K], G[K];
    load_points<K, true>(p, pos, stride, t, 0u, Slots{}, table);
    term<K, true>(p, L, gout[(size_t)t * gstride], G);
    float *c = contrib + (size_t)t * K * 3;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        c[k * 3 + 0] = G[k].x;
        c[k * 3 + 1] = G[k].y;
        c[k * 3 + 2] = G[k].z;
    }
}

// CG mode, pass 2: one lane per row sums its contribution rows in ascending order (every row written)
__global__ __launch_bounds__(256) void geom_cg_gather_kernel(unsigned B, const int *__restrict__ bead_ptr,
                                                             const int *__restrict__ bead_rows, const float *__restrict__ contrib,
                                                             float *__restrict__ gpos) {
    const unsigned b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float x = 0.f, y = 0.f, z = 0.f;
    const int end = bead_ptr[b + 1];
    for (int k = bead_ptr[b]; k < end; ++k) {
        const float *c = contrib + (size_t)bead_rows[k] * 3;
        x += c[0];
        y += c[1];
        z += c[2];
    }
    gpos[(size_t)b * 3 + 0] = x;
    gpos[(size_t)b * 3 + 1] = y;
    gpos[(size_t)b * 3 + 2] = z;
}

inline dim3 blocks_for(unsigned n) { return dim3((n + 255u) / 256u); }

// the K slots of a molecule term: in [0, MN), all different
int check_slots(const char *fn, unsigned MN, unsigned K, const Slots &sl) {
    for (unsigned k = 0; k < K; ++k) {
        HTF_REQUIRE(sl.s[k] >= 0 && (unsigned)sl.s[k] < MN, "%s: slot %d out of [0, %u)", fn, sl.s[k], MN);
        for (unsigned q = 0; q < k; ++q) HTF_REQUIRE(sl.s[q] != sl.s[k], "%s: slot %d repeated", fn, sl.s[k]);
    }
    return HTF_OK;
}

} // namespace

#define HTF_GEOM_DISPATCH(K, LAUNCH)                                                                                        \
    switch (K) {                                                                                                            \
    case 2: LAUNCH(2); break;                                                                                               \
    case 3: LAUNCH(3); break;                                                                                               \
    default: LAUNCH(4); break;                                                                                              \
    }

extern "C" int htf_geom_mol_forward(const float *d_pos, unsigned pos_stride, unsigned M, unsigned MN, unsigned K, int s0, int s1,
                                    int s2, int s3, const float *d_box_L, float *d_out, htf_stream stream) {
    HTF_REQUIRE(K >= 2 && K <= 4, "htf_geom_mol_forward: K must be 2, 3 or 4 (got %u)", K);
    HTF_REQUIRE(pos_stride >= 3, "htf_geom_mol_forward: pos_stride must be >= 3 (got %u)", pos_stride);
    const Slots sl = {{s0, s1, s2, s3}};
    if (int rc = check_slots("htf_geom_mol_forward", MN, K, sl)) return rc;
    if (M == 0) return HTF_OK;
    HTF_REQUIRE(d_pos && d_box_L && d_out, "htf_geom_mol_forward: null pointer");
    const hipStream_t s = (hipStream_t)stream;
#define HTF_LAUNCH(KK) hipLaunchKernelGGL((geom_forward_kernel<KK, false>), blocks_for(M), dim3(256), 0, s, d_pos, pos_stride, M, MN, \
                                          sl, nullptr, d_box_L, d_out)
    HTF_GEOM_DISPATCH(K, HTF_LAUNCH)
#undef HTF_LAUNCH
    return htf::check_launch("geom_forward_kernel");
}

extern "C" int htf_geom_mol_backward(const float *d_pos, unsigned pos_stride, unsigned M, unsigned MN, unsigned K, int s0, int s1,
                                     int s2, int s3, const float *d_box_L, const float *d_grad_out, unsigned grad_stride,
                                     float *d_grad_pos, htf_stream stream) {
    HTF_REQUIRE(K >= 2 && K <= 4, "htf_geom_mol_backward: K must be 2, 3 or 4 (got %u)", K);
    HTF_REQUIRE(pos_stride >= 3, "htf_geom_mol_backward: pos_stride must be >= 3 (got %u)", pos_stride);
    const Slots sl = {{s0, s1, s2, s3}};
    if (int rc = check_slots("htf_geom_mol_backward", MN, K, sl)) return rc;
    if (M == 0) return HTF_OK;
    HTF_REQUIRE(d_pos && d_box_L && d_grad_out && d_grad_pos, "htf_geom_mol_backward: null pointer");
    const hipStream_t s = (hipStream_t)stream;
#define HTF_LAUNCH(KK) hipLaunchKernelGGL(geom_mol_backward_kernel<KK>, blocks_for(M), dim3(256), 0, s, d_pos, pos_stride, M, MN, sl, \
                                          d_box_L, d_grad_out, grad_stride, d_grad_pos)
    HTF_GEOM_DISPATCH(K, HTF_LAUNCH)
#undef HTF_LAUNCH
    return htf::check_launch("geom_mol_backward_kernel");
}

extern "C" int htf_geom_cg_forward(const float *d_pos, unsigned pos_stride, unsigned B, unsigned K, unsigned T, const int *d_table,
                                   const float *d_box_L, float *d_out, htf_stream stream) {
    HTF_REQUIRE(K >= 2 && K <= 4, "htf_geom_cg_forward: K must be 2, 3 or 4 (got %u)", K);
    HTF_REQUIRE(pos_stride >= 3, "htf_geom_cg_forward: pos_stride must be >= 3 (got %u)", pos_stride);
    if (T == 0) return HTF_OK;
    HTF_REQUIRE(B > 0, "htf_geom_cg_forward: %u terms need rows", T);
    HTF_REQUIRE(d_pos && d_table && d_box_L && d_out, "htf_geom_cg_forward: null pointer");
    const hipStream_t s = (hipStream_t)stream;
#define HTF_LAUNCH(KK) hipLaunchKernelGGL((geom_forward_kernel<KK, true>), blocks_for(T), dim3(256), 0, s, d_pos, pos_stride, T, 0u, \
                                          Slots{}, d_table, d_box_L, d_out)
    HTF_GEOM_DISPATCH(K, HTF_LAUNCH)
#undef HTF_LAUNCH
    return htf::check_launch("geom_forward_kernel");
}

extern "C" int htf_geom_cg_backward(const float *d_pos, unsigned pos_stride, unsigned B, unsigned K, unsigned T, const int *d_table,
                                    const int *d_bead_ptr, const int *d_bead_rows, const float *d_box_L, const float *d_grad_out,
                                    unsigned grad_stride, float *d_contrib, float *d_grad_pos, htf_stream stream) {
    HTF_REQUIRE(K >= 2 && K <= 4, "htf_geom_cg_backward: K must be 2, 3 or 4 (got %u)", K);
    HTF_REQUIRE(pos_stride >= 3, "htf_geom_cg_backward: pos_stride must be >= 3 (got %u)", pos_stride);
    if (B == 0) return HTF_OK;
    HTF_REQUIRE(d_bead_ptr && d_grad_pos, "htf_geom_cg_backward: null pointer");
    const hipStream_t s = (hipStream_t)stream;
    if (T > 0) {
        HTF_REQUIRE(d_pos && d_table && d_bead_rows && d_box_L && d_grad_out && d_contrib, "htf_geom_cg_backward: null pointer");
#define HTF_LAUNCH(KK) hipLaunchKernelGGL(geom_cg_contrib_kernel<KK>, blocks_for(T), dim3(256), 0, s, d_pos, pos_stride, T, d_table, \
                                          d_box_L, d_grad_out, grad_stride, d_contrib)
        HTF_GEOM_DISPATCH(K, HTF_LAUNCH)
#undef HTF_LAUNCH
        if (int rc = htf::check_launch("geom_cg_contrib_kernel")) return rc;
    }
    hipLaunchKernelGGL(geom_cg_gather_kernel, blocks_for(B), dim3(256), 0, s, B, d_bead_ptr, d_bead_rows, d_contrib, d_grad_pos);
    return htf::check_launch("geom_cg_gather_kernel");
}
