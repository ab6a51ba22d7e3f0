/* htf_geom.h -- molecular geometry ops (utils.mol_bond_distance, mol_angle, mol_dihedral of hoomd-tf) on the device.
 *
 * Per-step model ops: the bond length, bond angle or dihedral of T terms of K = 2, 3 or 4 points each, and their
 * backward passes, so an energy of these values gives forces.  Same library (libhtf_amd.so), same status codes
 * (htf_amd.h), fp32 arrays, every pointer a device pointer unless stated.  Kept out of htf_amd.h (not part of the HOOMD
 * force-compute boundary) and out of htf_cg.h (the coarse-grained mapping ops).
 *
 * Point s of term t is row r of d_pos, its xyz at d_pos[r*pos_stride + 0..2].  Every vector between two points is
 * minimum-imaged in the orthorhombic box d_box_L = [Lx, Ly, Lz]: d - rint(d / L) L.
 *   K = 2 (bond):     d = p1 - p0; value |d|.
 *   K = 3 (angle):    a = p0 - p1, b = p2 - p1; value atan2(|a x b|, a . b) in [0, pi].
 *   K = 4 (dihedral): b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2, n1 = b1 x b2, n2 = b2 x b3;
 *                     value |atan2(|b2| b1 . n2, n1 . n2)| in [0, pi], and 0 where n1 = 0 or n2 = 0.
 * Degenerate terms (a bond of length 0, an angle with |a x b| = 0, a dihedral with n1 = 0 or n2 = 0) have a finite
 * value and a zero gradient.
 *
 * Molecule mode (htf_geom_mol_*): M molecules of MN rows each; point s of term t (= molecule t) is row t*MN + slot_s,
 * slots in [0, MN) and all different (s3 is ignored for K < 4, s2 for K < 3).
 * CG mode (htf_geom_cg_*): B rows; point s of term t is row d_table[t*K + s], every entry in [0, B) (not checked here).
 */
#ifndef HTF_GEOM_H_
#define HTF_GEOM_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* d_out [M]: the value of each molecule's term. */
HTF_API int htf_geom_mol_forward(const float *d_pos, unsigned pos_stride, unsigned M, unsigned MN, unsigned K, int s0, int s1,
                                 int s2, int s3, const float *d_box_L, float *d_out, htf_stream stream);

/* d_grad_pos [M*MN*3] = d value / d p, times d_grad_out[t*grad_stride] (grad_stride 0: one value for every term).  Every
 * row is written: the K rows of molecule t receive its term's gradient, the other rows zeros (no accumulation). */
HTF_API int htf_geom_mol_backward(const float *d_pos, unsigned pos_stride, unsigned M, unsigned MN, unsigned K, int s0, int s1,
                                  int s2, int s3, const float *d_box_L, const float *d_grad_out, unsigned grad_stride,
                                  float *d_grad_pos, htf_stream stream);

/* d_out [T]: the value of each term of the [T, K] table. */
HTF_API int htf_geom_cg_forward(const float *d_pos, unsigned pos_stride, unsigned B, unsigned K, unsigned T, const int *d_table,
                                const float *d_box_L, float *d_out, htf_stream stream);

/* Two passes, no atomics.  First each term t stores the gradient of its point s in d_contrib[(t*K + s)*3 + 0..2]
 * ([T*K*3], scratch).  Then each row b sums its contribution rows d_bead_rows[d_bead_ptr[b] .. d_bead_ptr[b+1]) in
 * that order into d_grad_pos[b*3 + 0..2] ([B*3], every row written).  d_bead_ptr [B+1] / d_bead_rows [T*K] is the
 * inverted index of d_table: the contribution rows t*K + s with d_table[t*K + s] = b.  Bitwise reproducible. */
HTF_API int htf_geom_cg_backward(const float *d_pos, unsigned pos_stride, unsigned B, unsigned K, unsigned T, const int *d_table,
                                 const int *d_bead_ptr, const int *d_bead_rows, const float *d_box_L, const float *d_grad_out,
                                 unsigned grad_stride, float *d_contrib, float *d_grad_pos, htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_GEOM_H_ */
