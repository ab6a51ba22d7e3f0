/* htf_ctrain.h -- force matching on the conservative forces of the descriptor network (htf.DescriptorMLP(trainable="total"),
 * DescriptorMLP.total_loss_gradient): the gradient, with respect to the weights, of the sum of squared residuals of
 * F = -d(sum_i E_i)/dr (htf_cforce.h) and E_i against the labels, in one sweep over the pair vectors.
 *
 * htf_bp_loss_grad (htf_bp.h) fits the row operator's 2 sum_j dE_i/dx_ij, a different function of the weights.  With the
 * residual rho_i = pred_i - labels_i held fixed ([B][4]: three force components and the energy residual rho_iE), collect
 * sum_i rho_i . F_i by the g_i = dE_i/dG_i it multiplies (F_i of htf_cforce.h holds g_i on row i's own slots and g_j on the
 * slots of the rows j that list i; renaming the second sum's rows puts every g_i on row i's slots):
 *
 *   Gdot_i[t K + k] = sum_s live_is [t_ij = t] R'_k(r_is) ((rho_i - m_is rho_j) . u_is)
 *   R'_k(r) = fc(r) c_der (r - mu_k) e_k(r) + fc'(r) e_k(r)
 *   u_is    = (x_ij + 1e-7) / r_is,   j = idx[i, s]
 *   m_is    = 1 if 0 <= j < B, else 0
 *   SSR     = sum_i |rho_i|^2 + rho_iE^2
 *   d SSR / d theta = 2 sum_i d( g_i . Gdot_i + rho_iE E_i ) / d theta                    (rho held fixed)
 *
 * with x_ij, r, live, t_ij, e_k, c_der, fc and fc' exactly those of htf_bp.h (live needs the neighbor type in range and, with
 * a cutoff, r < r_cut); no factor 2 inside Gdot.  This is the sweep of htf_bp_loss_grad with a = ((rho_i - m rho_j) . t) / r
 * in place of a = 2 (rho_i . t) / r: the same forward pass carrying (value, tangent), the same reverse pass, the same block
 * partials and the same fixed-order reduction.  The term of row i goes to the network that evaluates row i, so one launch per
 * species (d_rows, d_weights as in htf_bp_forces) covers several networks; the rows' own types are not needed.
 *
 * The regrouping is exact: Gdot is the adjoint of htf_cf_forces' F for any list, symmetric or not, and for any types.  Where
 * the list is symmetric within the descriptor's range (htf_cforce.h) it is the gradient of the fit to -d(sum_i E_i)/dr.
 *
 * Every term lands on the row that reads it: no atomics, no scatter.  Per live slot the sweep reads one int32 of d_index and
 * gathers one 16-byte row of d_rho; an index outside [0, B) has m = 0 and nothing is read for it.
 *
 * Bit contracts: (a) two calls on the same inputs give the same bits; (b) list entry q is accumulated by the wave and block
 * that q alone decides (d_rho and d_index are read at the ROW d_rows[q]).  Same library, status codes and enums as htf_amd.h;
 * every pointer is a device pointer.
 */
#ifndef HTF_CTRAIN_H_
#define HTF_CTRAIN_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* d_index [B][NN] int32: the particle in each slot (htf_cf_pair_index; any value on a slot that is not live).  d_rho [B][4]
 * fp32: the residual (F_i - F_i^label, E_i - E_i^label) of EVERY row, listed or not: a listed row gathers its neighbors'.
 * d_accum [1 + P] floats receives {sum over the listed rows of |rho_i|^2, d SSR / d theta_0, ...}, the convention of
 * htf_bp_loss_grad; it is OVERWRITTEN (n_rows = 0: the sweep is not launched and d_accum receives zeros; B = 0: d_accum may
 * be NULL, and then nothing is launched).  d_scratch: at least htf_bp_scratch_floats(n_rows, ...) floats.  d_rows, n_rows,
 * r_cut, d_weights and the limits as in htf_bp_loss_grad. */
HTF_API int htf_ct_loss_grad(const void *d_nlist, int nlist_dtype, const int *d_index, unsigned B, unsigned NN, unsigned K,
                             unsigned n_types, unsigned H1, unsigned H2, int activation, const float *d_weights, const float *d_mu,
                             float gap, const float *d_rho, float *d_accum, float *d_scratch, const int *d_rows, unsigned n_rows,
                             float r_cut, htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_CTRAIN_H_ */
