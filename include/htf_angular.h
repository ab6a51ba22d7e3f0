/* htf_angular.h -- angular channels of the descriptor network on its conservative forces
 * (htf.DescriptorMLP(conservative=True, l_max=1 or 2)).
 *
 * htf_bp.h's descriptor G_i sees neighbor distances only.  With l_max >= 1 the network also reads, per channel c = t K + k
 * (Dr = n_types K of them), invariants of the neighbors' moment tensors:
 *
 *   w_k(r)  = fc(r) e_k(r)                                    u_ij = (x_ij + 1e-7) / r_ij
 *   G_i[c]  = sum_j live [t_ij = t] w_k(r_ij)                                   (htf_bp.h)
 *   v_i[c]  = sum_j live [t_ij = t] w_k(r_ij) u_ij                              l_max >= 1
 *   M_i[c]  = sum_j live [t_ij = t] w_k(r_ij) u_ij (outer) u_ij                 l_max  = 2
 *   A_i[c]  = |v_i[c]|^2     = sum_jj' w w' cos(theta_jij')
 *   Q_i[c]  = ||M_i[c]||_F^2 = sum_jj' w w' cos^2(theta_jij')
 *
 * with x_ij, r_ij, live, t_ij, e_k, fc exactly those of htf_bp.h.  The network input is [G | A | Q], D = Dr (1 + l_max) <= 64
 * values, each block in channel order; E_i is htf_bp.h's three-layer network on it (weights of a network with D inputs).
 *
 * Forces are those of the total energy, F = -d(sum_i E_i)/dr, in the two sweeps of htf_cforce.h.  With g = dE_i/d(input),
 * p_i[c] = 2 g_i[Dr + c] v_i[c], S_i[c] = 2 g_i[2 Dr + c] M_i[c], j = idx[i, s], t_j the slot's type, t_i the row's own,
 * w_k' = fc c_der (r - mu_k) e_k + fc' e_k:
 *
 *   s0_k   = g_i[t_j K + k] + g_j[t_i K + k]
 *   dp_k   = p_i[t_j K + k] - p_j[t_i K + k]
 *   sS_k   = S_i[t_j K + k] + S_j[t_i K + k]
 *   phi_is = sum_k w_k' (s0_k + dp_k.u + u.sS_k u) u + (1/r) sum_k w_k [ (dp_k - (dp_k.u) u) + 2 (sS_k u - (u.sS_k u) u) ]
 *   F_i    = sum_s live_is phi_is,     W_i = -1/2 sum_s live_is x_ij (outer) phi_is     (a general 3x3)
 *
 * The reverse terms (index j) are taken at row i's own r and u and change sign with the parity of l.  They are dropped as in
 * htf_cforce.h: a neighbor type outside [0, n_types) empties the slot's own-row terms only; an index outside [0, B), or an own
 * type out of range, drops the reverse terms.  F is the gradient when the list is symmetric within the descriptor's range.
 *
 * Pass 1 writes, per row and channel, C = 4 (l_max = 1) or 10 (l_max = 2) floats {g, p, S} (S as xx, xy, xz, yy, yz, zz) to a
 * table h [B][Dr][C]; pass 2 gathers K C contiguous floats of it per slot.  No atomics: a row's bits depend on its slots,
 * its indices and the gathered table rows alone.  l_max = 0 is htf_cforce.h and is refused here.  Same library, status codes
 * and enums as htf_amd.h; every pointer is a device pointer.
 */
#ifndef HTF_ANGULAR_H_
#define HTF_ANGULAR_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Pass 1: htf_cf_grad's arguments, l_max (1 or 2) and the table.  d_weights: one network of D = K n_types (1 + l_max) inputs.
 * d_table [B][K n_types][C] fp32, 16-byte aligned, and d_energy [B] fp32 are written for the rows listed (d_rows, n_rows as
 * in htf_bp_forces: one launch per species present).  B = 0 or n_rows = 0 launches nothing. */
HTF_API int htf_ang_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types, unsigned H1,
                         unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap, float *d_table,
                         float *d_energy, const int *d_rows, unsigned n_rows, float r_cut, unsigned l_max, htf_stream stream);

/* Pass 2, every row in one launch: htf_cf_forces' arguments with the table in place of g, and l_max.  d_force [B][4]
 * (force_dtype): (F_i, E_i).  d_virial9, if not NULL, [B][9] (force_dtype): W_i, row-major. */
HTF_API int htf_ang_forces(const void *d_nlist, int nlist_dtype, const int *d_index, const float *d_types, unsigned B, unsigned NN,
                           unsigned K, unsigned n_types, const float *d_mu, float gap, const float *d_table, const float *d_energy,
                           void *d_force, int force_dtype, void *d_virial9, float r_cut, unsigned l_max, htf_stream stream);

/* The network input alone: d_out [B][D] (out_dtype) receives [G | A | Q], the bits pass 1 feeds the network. */
HTF_API int htf_ang_descriptor(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types,
                               const float *d_mu, float gap, void *d_out, int out_dtype, float r_cut, unsigned l_max,
                               htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_ANGULAR_H_ */
