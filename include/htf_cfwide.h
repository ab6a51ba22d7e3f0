/* htf_cfwide.h -- pass 1 of the conservative forces (htf_cforce.h) for networks with hidden layers up to 256 wide
 * (htf.DescriptorMLP(conservative=True, dense="mfma")): the dense stack on the fp32 matrix instruction.
 *
 * htf_cf_grad keeps one hidden unit per lane and so ends at 64 units.  This entry writes the same two tables,
 *
 *   d_g [B][D]   g_i = dE_i/dG_i          d_energy [B]   E_i = W3^T act(W2^T act(W1^T G_i + b1) + b2) + b3
 *
 * for a network of 1 <= H1, H2 <= 256, a tile of 64 rows at a time: G_i by the row kernel's own sums (the bits of
 * htf_bp_descriptor), then forward and backward of the whole tile as matrix products in exact fp32.  Pass 2 (htf_cf_forces,
 * htf_cf_forces_ghost) reads only g and E and serves both entries.  The descriptor's limits are htf_cforce.h's:
 * K * n_types <= 64, NN <= 256.  g and E agree with htf_cf_grad's to rounding, not bit for bit: the sums over the hidden
 * units run in the matrix unit's order.  No atomics: a row's values depend on its slots and the weights alone, not on the tile
 * or the batch it is evaluated in.  Same library, status codes and enums as htf_amd.h; every pointer is a device pointer.
 */
#ifndef HTF_CFWIDE_H_
#define HTF_CFWIDE_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HTF_CFW_MAX_H 256u
/* dynamic LDS of a launch: 4 (65 (D32 + H1_32 + H2_32) + 4 H2_32 + K4 + 64) bytes, widths rounded up to multiples of 32 and K
 * to a multiple of 4; 154 368 bytes at the limits.  Above this the call returns HTF_ERR_INVALID and launches nothing. */
#define HTF_CFW_MAX_LDS_BYTES (160u * 1024u)

/* Argument for argument htf_cf_grad (htf_cforce.h), with H1, H2 <= HTF_CFW_MAX_H: d_g [B][D] and d_energy [B] fp32 are
 * written for the rows listed (d_rows, n_rows; NULL: rows 0 .. n_rows - 1), one launch per species present.  d_weights: one
 * network, Keras order, unpadded.  B = 0 or n_rows = 0 launches nothing. */
HTF_API int htf_cfw_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types, unsigned H1,
                         unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap, float *d_g,
                         float *d_energy, const int *d_rows, unsigned n_rows, float r_cut, htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_CFWIDE_H_ */
