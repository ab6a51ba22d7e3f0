/* htf_cg.h -- coarse-grained mapping ops (utils.center_of_mass, utils.compute_nlist of hoomd-tf) on the device.
 *
 * Per-step model ops a coarse-grained model calls inside SimModel.compute: the periodic centre of mass of the
 * beads of a sparse B x N mapping, and an all-pairs neighbor list of the beads.  Both have their backward pass
 * here, so a CG energy gives atom forces.  Same library (libhtf_amd.so), same status codes (htf_amd.h), fp32
 * arrays, every pointer a device pointer unless stated.  Kept out of htf_amd.h: these ops are not part of the
 * HOOMD force-compute boundary that header describes.
 */
#ifndef HTF_CG_H_
#define HTF_CG_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Largest NN htf_cg_nlist_forward accepts. */
#define HTF_CG_MAX_NN 256

/* Centre of mass, per bead b and component c (L = d_box_L[c], theta = 2 pi p / L):
 *   X = sum_a w_ab cos(theta_ac), Z = sum_a w_ab sin(theta_ac), com[b*3+c] = atan2(Z, X) L / (2 pi), in (-L/2, L/2].
 * d_pos: atom a's xyz at d_pos[a*pos_stride + 0..2].  The mapping as CSR: d_row_ptr [B+1], d_cols / d_vals [nnz],
 * atom indices < N.  d_xz (nullable) [B*6] receives X (first three) and Z (last three) of each bead, for the backward. */
HTF_API int htf_cg_com_forward(const float *d_pos, unsigned pos_stride, unsigned N, unsigned B, const int *d_row_ptr,
                               const int *d_cols, const float *d_vals, const float *d_box_L, float *d_com, float *d_xz,
                               htf_stream stream);

/* d grad_pos[a*3+c] = sum_b w_ab (X_bc cos theta_ac + Z_bc sin theta_ac) / (X_bc^2 + Z_bc^2) * d_grad_com[b*3+c]
 * (0 where X^2 + Z^2 = 0).  The mapping as CSC: d_col_ptr [N+1], d_rows / d_vals [nnz].  Every atom is written
 * (no accumulation, no atomics): deterministic. */
HTF_API int htf_cg_com_backward(const float *d_pos, unsigned pos_stride, unsigned N, unsigned B, const int *d_col_ptr,
                                const int *d_rows, const float *d_vals, const float *d_box_L, const float *d_xz,
                                const float *d_grad_com, float *d_grad_pos, htf_stream stream);

/* All-pairs neighbor list of M particles (utils.compute_nlist): r_ij = minimage(p_j - p_i) (round half to even),
 * d = |r_ij|, j a neighbor of i when 5e-4 <= d <= r_cut and neither d_excl[i*M+j] nor d_excl[j*M+i] is set
 * (d_excl nullable, one byte per pair).  sorted != 0: the NN nearest, nearest first; sorted = 0: the NN farthest,
 * farthest first; ties to the lower index in both.  d_out [M*NN*4]: (r_ij, j) -- or (r_ij, d_pos[j*pos_stride+3])
 * when return_types != 0 -- and zeros in empty slots; d_idx [M*NN]: j, or -1 in empty slots.  1 <= NN <= HTF_CG_MAX_NN.
 * Cost grows as M^2 (no cell search). */
HTF_API int htf_cg_nlist_forward(const float *d_pos, unsigned pos_stride, unsigned M, const float *d_box_L, float r_cut,
                                 unsigned NN, int sorted, int return_types, const unsigned char *d_excl, float *d_out,
                                 int *d_idx, htf_stream stream);

/* Backward of the xyz of htf_cg_nlist_forward: for every filled slot (i, s) with j = d_idx[i*NN+s] and
 * g = d_grad_out[(i*NN+s)*4 + 0..2]: grad_pos[i] -= g, grad_pos[j] += g.  d_grad_pos [M*3] accumulates (atomics):
 * the caller zeroes it. */
HTF_API int htf_cg_nlist_backward(const int *d_idx, unsigned M, unsigned NN, const float *d_grad_out, float *d_grad_pos,
                                  htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_CG_H_ */
