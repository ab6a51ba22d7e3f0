/* htf_atrain.h -- force matching on the conservative forces of the descriptor network with angular channels
 * (htf.DescriptorMLP(l_max=1 or 2, trainable="angular"), DescriptorMLP.angular_loss_gradient): the gradient, with respect to
 * the weights, of the sum of squared residuals of F = -d(sum_i E_i)/dr (htf_angular.h) and E_i against the labels, in one sweep
 * over the pair vectors.
 *
 * htf_ct_loss_grad (htf_ctrain.h) is the sweep for l_max = 0.  With the residual rho_i = pred_i - labels_i held fixed ([B][4]:
 * three force components and the energy residual rho_iE), displacing every particle by eps rho changes the pair vector of slot
 * s of row i by eps (m_is rho_j - rho_i), and rho . F = -D_rho(sum_i E_i): sum_i rho_i . F_i is, row by row, the derivative of
 * E_i along a tangent of its own input X_i = [G | A | Q].  With live, t_ij, w_k = fc e_k, v, M, A and Q those of htf_angular.h,
 * w_k' = fc c_der (r - mu_k) e_k + fc' e_k, u = (x + 1e-7) / r, j = idx[i, s] and m_is = 1 if 0 <= j < B, else 0:
 *
 *   d_is  = rho_i - m_is rho_j                      (the three force components)
 *   a     = d_is . u,    dperp = d_is - a u
 *   Gdot_i[c] = sum_s [t_is = t] w_k' a
 *   vdot_i[c] = sum_s [t_is = t] ( w_k' a u + (w_k / r) dperp )
 *   Mdot_i[c] = sum_s [t_is = t] ( w_k' a u (outer) u + (w_k / r) (dperp (outer) u + u (outer) dperp) )
 *   Adot = 2 v . vdot,    Qdot = 2 M : Mdot         (M symmetric: the off-diagonals count twice, as in Q)
 *   SSR  = sum_i |rho_i|^2 + rho_iE^2
 *   d SSR / d theta = 2 sum_i d( grad_X E_i . Xdot_i + rho_iE E_i ) / d theta,   Xdot = [Gdot | Adot | Qdot]   (rho held fixed)
 *
 * This is the sweep of htf_bp_loss_grad and htf_ct_loss_grad over D = K n_types (1 + l_max) inputs: the same forward pass
 * carrying (value, tangent), the same reverse pass, the same block partials and the same fixed-order reduction.  The term of
 * row i goes to the network that evaluates row i, so one launch per species (d_rows, d_weights as in htf_bp_forces) covers
 * several networks; the rows' own types are not needed.
 *
 * The regrouping is exact: Xdot is the adjoint of htf_ang_forces' F for a list that is symmetric within the descriptor's range
 * (htf_cforce.h), and there it is the gradient of the fit to -d(sum_i E_i)/dr.  A slot whose index is outside [0, B) has no
 * rho_j, as it has no reverse term in htf_ang_forces.
 *
 * Every term lands on the row that reads it: no atomics, no scatter.  Per live slot the sweep reads one int32 of d_index and
 * gathers one 16-byte row of d_rho; an index outside [0, B) has m = 0 and nothing is read for it.
 *
 * Bit contracts: (a) two calls on the same inputs give the same bits; (b) list entry q is accumulated by the wave and block
 * that q alone decides (d_rho and d_index are read at the ROW d_rows[q]).  Same library, status codes and enums as htf_amd.h;
 * every pointer is a device pointer.
 */
#ifndef HTF_ATRAIN_H_
#define HTF_ATRAIN_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The arguments of htf_ct_loss_grad, and l_max = 1 or 2 (0: htf_ct_loss_grad) with K n_types (1 + l_max) <= 64.  d_weights:
 * the network of D = K n_types (1 + l_max) inputs; d_accum [1 + P] floats, P = D H1 + H1 + H1 H2 + H2 + H2 + 1, is
 * OVERWRITTEN (n_rows = 0: the sweep is not launched and d_accum receives zeros; B = 0: d_accum may be NULL, and then nothing
 * is launched).  d_scratch: at least htf_bp_scratch_floats(n_rows, K, n_types (1 + l_max), H1, H2) floats. */
HTF_API int htf_at_loss_grad(const void *d_nlist, int nlist_dtype, const int *d_index, unsigned B, unsigned NN, unsigned K,
                             unsigned n_types, unsigned H1, unsigned H2, int activation, const float *d_weights, const float *d_mu,
                             float gap, const float *d_rho, float *d_accum, float *d_scratch, const int *d_rows, unsigned n_rows,
                             float r_cut, unsigned l_max, htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_ATRAIN_H_ */
