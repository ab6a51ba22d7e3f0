/* htf_cfwide3.h -- pass 1 of the conservative forces (htf_cforce.h) for networks with three hidden layers up to 256 wide
 * (htf.DescriptorMLP(conservative=True, dense="mfma", H3=...)): the dense stack on the fp32 matrix instruction.
 *
 * htf_cfw_grad (htf_cfwide.h) evaluates D -> H1 -> H2 -> 1.  This entry writes the same two tables,
 *
 *   d_g [B][D]   g_i = dE_i/dG_i      d_energy [B]   E_i = W4^T act(W3^T act(W2^T act(W1^T G_i + b1) + b2) + b3) + b4
 *
 * for 1 <= H1, H2, H3 <= 256: G_i by the row kernel's own sums (the bits of htf_bp_descriptor), then forward and backward of
 * a whole tile of rows as matrix products in exact fp32.  Pass 2 (htf_cf_forces, htf_cf_forces_ghost) reads only g and E and
 * serves this entry as it serves htf_cf_grad and htf_cfw_grad.  The descriptor's limits are htf_cforce.h's: K * n_types <= 64,
 * NN <= 256.  No atomics: a row's values depend on its slots and the weights alone, not on the tile or the batch it is
 * evaluated in.  Evaluation only: the force-matching sweep for three hidden layers is a follow-up.  Same library, status codes
 * and enums as htf_amd.h; every pointer is a device pointer.
 *
 * LDS.  A tile keeps three images, one line of R floats per feature, lines R + 1 floats apart:
 *
 *   XA [max(D32, H3_32)]  G, then dz3, then g        A1 [H1_32]  h1, then dz1        A2 [H2_32]  h2, then dz2
 *
 * (widths rounded up to multiples of 32; G is dead once h1 exists and g is written after dz3's last use, so dz3 shares their
 * lines), and beside them the energy's partials, the centres and the tile's rows:
 *
 *   bytes(R) = 4 ((R + 1) (max(D32, H3_32) + H1_32 + H2_32) + 2 R H3_32 / 32 + K4 + R)        K4: K rounded up to 4
 *
 * The rule: R = 64 while bytes(64) <= HTF_CFW3_MAX_LDS_BYTES, else R = 32.  With K = 16, bytes(64) is 25 792 at 16 x 32 x 32 x 32,
 * 101 696 at 16 x 160 x 128 x 96 and 137 536 at 16 x 128 x 128 x 256; at 64 x 256 x 256 x 256 it would be 204 096, and the
 * 32-row tile takes 103 616 there (103 808 with K = 64, the largest any network needs).  Every width triple in [1, 256]^3
 * with D <= 64 launches.
 */
#ifndef HTF_CFWIDE3_H_
#define HTF_CFWIDE3_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HTF_CFW3_MAX_H 256u
#define HTF_CFW3_MAX_LDS_BYTES (160u * 1024u)

/* htf_cfw_grad's arguments (htf_cfwide.h) with H3 after H2: d_g [B][D] and d_energy [B] fp32 are written for the rows listed
 * (d_rows, n_rows; NULL: rows 0 .. n_rows - 1), one launch per species present.  d_weights: one network of
 * D H1 + H1 + H1 H2 + H2 + H2 H3 + H3 + H3 + 1 floats, Keras order (W1, b1, W2, b2, W3, b3, W4, b4), unpadded.
 * B = 0 or n_rows = 0 launches nothing. */
HTF_API int htf_cfw3_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types, unsigned H1,
                          unsigned H2, unsigned H3, int activation, const float *d_weights, const float *d_mu, float gap,
                          float *d_g, float *d_energy, const int *d_rows, unsigned n_rows, float r_cut, htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_CFWIDE3_H_ */
