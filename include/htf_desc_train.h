/* htf_desc_train.h -- force matching for the descriptor network (htf.DescriptorMLP(trainable=True)) on the device.
 *
 * One sweep over the [B, NN, 4] pair-vector tensor gives the sum of squared residuals of the network's prediction
 * (F_i, E_i) (htf_desc.h) against the labels, and its gradient with respect to the network's weights:
 *
 *   rho_i = pred_i - labels_i                                     ([B][4]: force residual and energy residual rho_iE)
 *   SSR   = sum_i |rho_i|^2 + rho_iE^2
 *   d SSR / d theta = 2 sum_i d (rho_i . F_i + rho_iE E_i) / d theta        (rho held fixed)
 *
 * rho_i . F_i is the network's directional derivative along Gdot_i[t*K + k] = sum_j live [t_ij = t] e_k'(r_ij) 2 (rho_i . t_ij) / r_ij
 * (t_ij = x_ij + 1e-7), so one forward pass carrying (value, tangent) and one reverse pass per row form the gradient; no
 * intermediate leaves the kernel.  Same library, status codes, dtype / activation enums and limits as htf_desc.h; every
 * pointer a device pointer.  Weights: W1 [D][H1] | b1 | W2 [H1][H2] | b2 | W3 [H2] | b3, P floats, the order of d_accum's
 * gradient.  The sweep uses no atomics: partial sums per block land in d_scratch and a second kernel adds them in a fixed
 * order, so two calls on the same inputs give the same bits.
 */
#ifndef HTF_DESC_TRAIN_H_
#define HTF_DESC_TRAIN_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* floats of d_scratch for a sweep over B rows (0 for B = 0) */
HTF_API size_t htf_dtrain_scratch_floats(unsigned B, unsigned K, unsigned n_types, unsigned H1, unsigned H2);

/* d_pred [B][4] fp32: the network's (F_i, E_i) at d_weights, as htf_desc_forces writes them.  d_labels [B][4]
 * (labels_dtype).  d_accum [1 + P] floats receives {SSR, d SSR / d theta_0, ...}, the convention of htf_train_pair_grad;
 * it is OVERWRITTEN (B = 0: zeros; it may then be NULL, and nothing is launched).  d_scratch: at least htf_dtrain_scratch_floats floats. */
HTF_API int htf_dtrain_loss_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types,
                                 unsigned H1, unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap,
                                 const void *d_labels, int labels_dtype, const float *d_pred, float *d_accum, float *d_scratch,
                                 htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_DESC_TRAIN_H_ */
