/* htf_desc.h -- the descriptor network (htf.DescriptorMLP) on the device.
 *
 * A per-particle energy of Behler-Parrinello / SchNet form: each row of the [B, NN, 4] pair-vector tensor (fp32 or fp64,
 * nlist_dtype) sums Gaussian radial channels of its neighbors into a descriptor G of D = n_types * K channels, and a
 * Dense(H1) -> Dense(H2) -> Dense(1) network turns G into the row's energy.  Same library (libhtf_amd.so), same status
 * codes and dtype / activation enums (htf_amd.h), every pointer a device pointer.  Kept out of htf_amd.h: not part of the
 * HOOMD force-compute boundary.
 *
 *   x_ij  = nlist[i, j, 0..2]
 *   r_ij  = sqrt(sum_c (x_ij,c + 1e-7)^2)                         (safe_norm)
 *   live  = r_ij > 3e-6                                           (the nlist_rinv criterion)
 *   t_ij  = 0 for n_types = 1, else rint(nlist[i, j, 3]); a type outside [0, n_types) contributes nothing
 *   G_i[t*K + k] = sum_j live [t_ij = t] exp(-(r_ij - d_mu[k])^2 / gap)
 *   E_i   = W3^T act(W2^T act(W1^T G_i + b1) + b2) + b3           (act: HTF_ACT_TANH or HTF_ACT_LINEAR)
 *
 * d_weights: W1 [D][H1] | b1 [H1] | W2 [H1][H2] | b2 [H2] | W3 [H2] | b3, row-major Keras kernels, fp32, read at every call.
 * d_mu: the K channel centres, fp32.  Limits: 2 <= K, D <= 64, 1 <= H1, H2 <= 64, NN <= 256, gap > 0.
 * Every row is independent of the others and of the batch it runs in; two calls give the same bits.
 */
#ifndef HTF_DESC_H_
#define HTF_DESC_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* d_force [B][4] (force_dtype): (f_i, E_i) with f_i = 2 sum_j dE_i / dx_ij.  d_virial9, if not NULL, [B][9] (force_dtype):
 * -sum_j |2 dE_i/dx_ij| / (2 |x_ij|) x_ij x_ij^T, the virial of the generic route. */
HTF_API int htf_desc_forces(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types,
                            unsigned H1, unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap,
                            void *d_force, int force_dtype, void *d_virial9, htf_stream stream);

/* d_out [B][D] (out_dtype): the descriptor G alone, the same bits the network of htf_desc_forces reads. */
HTF_API int htf_desc_descriptor(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types,
                                const float *d_mu, float gap, void *d_out, int out_dtype, htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_DESC_H_ */
