/* htf_bp.h -- the descriptor network with a smooth cutoff and over a row list (htf.DescriptorMLP(r_cut=..., n_species=...)).
 *
 * The entry points of htf_desc.h and htf_desc_train.h with three more arguments; everything those headers say holds here.
 *
 *   r_cut   0: none.  Otherwise every Gaussian is multiplied by the cosine cutoff of Behler and Parrinello,
 *             fc(r) = 0.5 (cos(pi r / r_cut) + 1) for r < r_cut, 0 for r >= r_cut           (r = r_ij, the fp32 safe_norm)
 *             G_i[t*K + k] = sum_j live [t_ij = t] fc(r_ij) exp(-(r_ij - d_mu[k])^2 / gap)
 *           and dG/dr gains the fc'(r) = -0.5 (pi / r_cut) sin(pi r / r_cut) term in the forces, the virial and the sweep.
 *           It should not exceed the cutoff of the neighbor list the pair vectors come from (not checked).
 *   d_rows  NULL, or n_rows int32 row indices in [0, B), each row at most once (not checked: the caller builds the list).
 *           Work item q handles row d_rows[q], or row q for NULL.  This is how one launch per particle species evaluates
 *           that species' rows with that species' d_weights.  Labels, d_pred and every output are indexed by the ROW;
 *           rows that are not listed are neither read nor written.
 *   n_rows  the number of work items, at most B.
 *
 * Bit contracts: (a) d_rows = NULL, n_rows = B, r_cut = 0 gives the bits of htf_desc_forces, htf_desc_descriptor and
 * htf_dtrain_loss_grad; (b) a row's force, energy, virial and descriptor bits depend on its slots, d_weights and r_cut alone,
 * not on the list, the batch or the launch; (c) the sweep treats list entry q exactly as row q of a call with B = n_rows, so
 * d_accum equals, bit for bit, the sweep over the gathered rows, labels and predictions.
 */
#ifndef HTF_BP_H_
#define HTF_BP_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* htf_desc_forces over a row list and with a cutoff */
HTF_API int htf_bp_forces(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types,
                          unsigned H1, unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap,
                          void *d_force, int force_dtype, void *d_virial9, const int *d_rows, unsigned n_rows, float r_cut,
                          htf_stream stream);

/* htf_desc_descriptor with a cutoff: the same G bits the network of htf_bp_forces reads at this r_cut */
HTF_API int htf_bp_descriptor(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types,
                              const float *d_mu, float gap, void *d_out, int out_dtype, float r_cut, htf_stream stream);

/* floats of d_scratch for a sweep over n_rows work items (0 for none): min(ceil(n_rows / 64), 512) partials of 1 + P */
HTF_API size_t htf_bp_scratch_floats(unsigned n_rows, unsigned K, unsigned n_types, unsigned H1, unsigned H2);

/* htf_dtrain_loss_grad over a row list and with a cutoff: d_accum [1 + P] is OVERWRITTEN with {SSR, d SSR / d theta} of the
 * listed rows (n_rows = 0: zeros; d_accum may then be NULL if B = 0, and nothing is launched). */
HTF_API int htf_bp_loss_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types,
                             unsigned H1, unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap,
                             const void *d_labels, int labels_dtype, const float *d_pred, float *d_accum, float *d_scratch,
                             const int *d_rows, unsigned n_rows, float r_cut, htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_BP_H_ */
