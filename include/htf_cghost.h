/* htf_cghost.h -- the conservative forces of the descriptor network and their force-matching sweeps on the rows of one domain
 * (htf.DescriptorMLP.total_forces / total_loss_gradient / angular_loss_gradient with n_ghost > 0; domain.SlabDomain.halo_rows).
 *
 * htf_cf_forces, htf_ang_forces, htf_ct_loss_grad and htf_at_loss_grad (htf_cforce.h, htf_angular.h, htf_ctrain.h,
 * htf_atrain.h) use one number B as the row count of the pair tensor and as the bound of a valid slot index.  Under domain
 * decomposition a rank owns B rows and its slots also name ghost particles, numbered from B up: copies of rows that a
 * neighboring rank owns.  What pass 2 and the sweeps gather per slot -- g_j = dE_j/dG_j, the {g, p, S} record of j, the
 * residual rho_j -- is a function of j's full neighborhood and is computed by the rank that owns j.  The entries below take
 * the gathered table with n_table >= B rows:
 *
 *   rows [0, B)        what this rank's own launches wrote (pass 1: htf_cf_grad, htf_ang_grad; the residual of its own rows)
 *   rows [B, n_table)  the ghosts' rows, copied from their owners between the two steps (one forward halo on the plan of the
 *                      position halo: 4 D, 16 Dr or 40 Dr bytes per ghost row, 16 for the residual)
 *
 * and read a slot's reverse term when 0 <= j < n_table.  Everything else is the twin entry's: the formulas, the live rule, the
 * keep rule, the types, the row list, the partials and the fixed-order reduction.  Row i's own g_i (own record, own residual)
 * is row i of the table; d_energy, d_force, d_virial9, d_types, d_nlist and d_index have B rows.  With n_table = B an entry
 * computes its twin's bits (the twins forward here); n_table < B is HTF_ERR_INVALID; B = 0 launches nothing.  No atomics: a
 * row's bits depend on its slots, its indices and the gathered rows alone, so a row computes the same bits whether its
 * neighbor's table row was written by a launch of this process or copied in.
 *
 * Same library, status codes and enums as htf_amd.h; every pointer is a device pointer.
 */
#ifndef HTF_CGHOST_H_
#define HTF_CGHOST_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* htf_cf_forces (htf_cforce.h) with d_g [n_table][D]. */
HTF_API int htf_cf_forces_ghost(const void *d_nlist, int nlist_dtype, const int *d_index, const float *d_types, unsigned B,
                                unsigned NN, unsigned K, unsigned n_types, const float *d_mu, float gap, const float *d_g,
                                const float *d_energy, void *d_force, int force_dtype, void *d_virial9, float r_cut,
                                unsigned n_table, htf_stream stream);

/* htf_ang_forces (htf_angular.h) with d_table [n_table][Dr][4 or 10]. */
HTF_API int htf_ang_forces_ghost(const void *d_nlist, int nlist_dtype, const int *d_index, const float *d_types, unsigned B,
                                 unsigned NN, unsigned K, unsigned n_types, const float *d_mu, float gap, const float *d_table,
                                 const float *d_energy, void *d_force, int force_dtype, void *d_virial9, float r_cut,
                                 unsigned l_max, unsigned n_table, htf_stream stream);

/* htf_ct_loss_grad (htf_ctrain.h) with d_rho [n_table][4]: m_is = 1 if 0 <= j < n_table.  d_rows lists rows of [0, B). */
HTF_API int htf_ct_loss_grad_ghost(const void *d_nlist, int nlist_dtype, const int *d_index, unsigned B, unsigned NN, unsigned K,
                                   unsigned n_types, unsigned H1, unsigned H2, int activation, const float *d_weights,
                                   const float *d_mu, float gap, const float *d_rho, float *d_accum, float *d_scratch,
                                   const int *d_rows, unsigned n_rows, float r_cut, unsigned n_table, htf_stream stream);

/* htf_at_loss_grad (htf_atrain.h) with d_rho [n_table][4]. */
HTF_API int htf_at_loss_grad_ghost(const void *d_nlist, int nlist_dtype, const int *d_index, unsigned B, unsigned NN, unsigned K,
                                   unsigned n_types, unsigned H1, unsigned H2, int activation, const float *d_weights,
                                   const float *d_mu, float gap, const float *d_rho, float *d_accum, float *d_scratch,
                                   const int *d_rows, unsigned n_rows, float r_cut, unsigned l_max, unsigned n_table,
                                   htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_CGHOST_H_ */
