/* htf_bp.h -- the descriptor network (htf.DescriptorMLP) on the device: forces, descriptor and force-matching sweep.
 *
 * A per-particle energy of Behler-Parrinello / SchNet form: each row of the [B, NN, 4] pair-vector tensor (fp32 or fp64,
 * nlist_dtype) sums Gaussian radial channels of its neighbors into a descriptor G of D = n_types * K channels, and a
 * Dense(H1) -> Dense(H2) -> Dense(1) network turns G into the row's energy.  Same library (libhtf_amd.so), same status
 * codes and dtype / activation enums (htf_amd.h), every pointer a device pointer.  Kept out of htf_amd.h: not part of the
 * HOOMD force-compute boundary.
 *
 *   x_ij  = nlist[i, j, 0..2]
 *   r_ij  = sqrt(sum_c (x_ij,c + 1e-7)^2)                         (safe_norm, in fp32)
 *   live  = r_ij > 3e-6                                           (the nlist_rinv criterion)
 *   t_ij  = 0 for n_types = 1, else rint(nlist[i, j, 3]); a type outside [0, n_types) contributes nothing
 *   G_i[t*K + k] = sum_j live [t_ij = t] fc(r_ij) exp(-(r_ij - d_mu[k])^2 / gap)
 *   E_i   = W3^T act(W2^T act(W1^T G_i + b1) + b2) + b3           (act: HTF_ACT_TANH or HTF_ACT_LINEAR)
 *
 * d_weights: W1 [D][H1] | b1 [H1] | W2 [H1][H2] | b2 [H2] | W3 [H2] | b3, row-major Keras kernels, P fp32 values, read at
 * every call.  d_mu: the K channel centres, fp32.  Limits: 2 <= K, D <= 64, 1 <= H1, H2 <= 64, NN <= 256, gap > 0.
 *
 *   r_cut   0: none, fc = 1.  Otherwise the cosine cutoff of Behler and Parrinello,
 *             fc(r) = 0.5 (cos(pi r / r_cut) + 1) for r < r_cut, 0 for r >= r_cut,
 *           and dG/dr gains the fc'(r) = -0.5 (pi / r_cut) sin(pi r / r_cut) term in the forces, the virial and the sweep.
 *           It should not exceed the cutoff of the neighbor list the pair vectors come from (not checked).
 *   d_rows  NULL, or n_rows int32 row indices in [0, B), each row at most once (not checked: the caller builds the list).
 *           Work item q handles row d_rows[q], or row q for NULL.  This is how one launch per particle species evaluates
 *           that species' rows with that species' d_weights.  Labels, d_pred and every output are indexed by the ROW;
 *           rows that are not listed are neither read nor written.
 *   n_rows  the number of work items, at most B (B itself for the whole batch without a list).
 *
 * Force matching: one sweep over the pair vectors gives the sum of squared residuals of the network's prediction
 * (F_i, E_i) against the labels, and its gradient with respect to d_weights:
 *
 *   rho_i = pred_i - labels_i                                     ([B][4]: force residual and energy residual rho_iE)
 *   SSR   = sum_i |rho_i|^2 + rho_iE^2
 *   d SSR / d theta = 2 sum_i d (rho_i . F_i + rho_iE E_i) / d theta        (rho held fixed)
 *
 * rho_i . F_i is the network's directional derivative along Gdot_i[t*K + k] = sum_j live [t_ij = t] e_k'(r_ij) 2 (rho_i . t_ij) / r_ij
 * (t_ij = x_ij + 1e-7), so one forward pass carrying (value, tangent) and one reverse pass per row form the gradient; no
 * intermediate leaves the kernel.  The sweep uses no atomics: partial sums per block land in d_scratch and a second kernel
 * adds them in a fixed order.
 *
 * Bit contracts: (a) two calls on the same inputs give the same bits; (b) a row's force, energy, virial and descriptor bits
 * depend on its slots, d_weights and r_cut alone, not on the list, the batch or the launch; (c) the sweep treats list entry q
 * exactly as row q of a call with B = n_rows, so d_accum equals, bit for bit, the sweep over the gathered rows, labels and
 * predictions.
 */
#ifndef HTF_BP_H_
#define HTF_BP_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* d_force [B][4] (force_dtype): (f_i, E_i) with f_i = 2 sum_j dE_i / dx_ij.  d_virial9, if not NULL, [B][9] (force_dtype):
 * -sum_j |2 dE_i/dx_ij| / (2 |x_ij|) x_ij x_ij^T, the virial of the generic route. */
HTF_API int htf_bp_forces(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types,
                          unsigned H1, unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap,
                          void *d_force, int force_dtype, void *d_virial9, const int *d_rows, unsigned n_rows, float r_cut,
                          htf_stream stream);

/* d_out [B][D] (out_dtype): the descriptor G alone, every row, the same bits the network of htf_bp_forces reads at this r_cut. */
HTF_API int htf_bp_descriptor(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types,
                              const float *d_mu, float gap, void *d_out, int out_dtype, float r_cut, htf_stream stream);

/* floats of d_scratch for a sweep over n_rows work items (0 for none): min(ceil(n_rows / 64), 512) partials of 1 + P */
HTF_API size_t htf_bp_scratch_floats(unsigned n_rows, unsigned K, unsigned n_types, unsigned H1, unsigned H2);

/* d_pred [B][4] fp32: the network's (F_i, E_i) at d_weights, as htf_bp_forces writes them.  d_labels [B][4] (labels_dtype).
 * d_accum [1 + P] floats receives {SSR, d SSR / d theta_0, ...} of the listed rows, the convention of htf_train_pair_grad;
 * it is OVERWRITTEN (n_rows = 0: zeros; d_accum may then be NULL if B = 0, and nothing is launched).  d_scratch: at least
 * htf_bp_scratch_floats(n_rows, ...) floats. */
HTF_API int htf_bp_loss_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types,
                             unsigned H1, unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap,
                             const void *d_labels, int labels_dtype, const float *d_pred, float *d_accum, float *d_scratch,
                             const int *d_rows, unsigned n_rows, float r_cut, htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_BP_H_ */
