/* htf_cfwide16.h -- pass 1 of the conservative forces (htf_cforce.h) for networks with hidden layers up to 256 wide, the dense
 * stack on the fp16 matrix instruction with split operands (htf.DescriptorMLP(conservative=True, dense="split16")).
 *
 * htf_cfw_grad (htf_cfwide.h) runs the dense stack of a 64-row tile on v_mfma_f32_32x32x2_f32, the slowest matrix rate of the
 * part.  This entry writes the same two tables,
 *
 *   d_g [B][D]   g_i = dE_i/dG_i          d_energy [B]   E_i = W3^T act(W2^T act(W1^T G_i + b1) + b2) + b3
 *
 * from the same tile with every operand of a product as x = hi + lo, hi = fp16(x), lo = fp16(x - hi), both rounded to nearest,
 * and three partial products lo_a hi_b + hi_a lo_b + hi_a hi_b on v_mfma_f32_32x32x16_f16 with fp32 accumulators -- the form
 * HTF_MLP_SPLIT16 has for the pair network.  G_i is formed by the row kernel's own sums (the bits of htf_bp_descriptor) before
 * it is split; the activation function, the energy and g itself are evaluated and kept in fp32, while the tile's images of h1,
 * dz2 and dz1 (and of G) lie in LDS as fp16 hi + lo pairs, being operands of the next product.  The weights are read as they
 * lie in d_weights, fp32, and split in registers: the call keeps no image of them and no state.  The backward operands are
 * scaled by the power of two that puts the largest |W3| into [32, 64) and g is scaled back, exactly (they stay inside fp16's
 * range while a row of |W2| sums to less than 1 000).  Pass 2 (htf_cf_forces, htf_cf_forces_ghost) reads only g and E and
 * serves this entry too.  The descriptor's limits are htf_cforce.h's: K * n_types <= 64, NN <= 256.
 *
 * Accuracy: a part keeps 11 bits and an absolute step of 2^-24 below 2^-14, so a product operand carries a relative error of
 * 2^-22 or an absolute one of 2^-25, whichever is larger; g and E agree with htf_cfw_grad's to the rounding of an fp32 chain
 * (tests/test_gpu_desc_split16.py holds both to the same bound).  Range: an operand with |x| > 65504 -- a weight, or with
 * activation "linear" a hidden value -- is outside fp16; its hi is an infinity, its lo the opposite one, and E_i (and g_i
 * where it depends on that operand) of the rows it enters are NaN or infinite, never a wrong finite value.
 *
 * No atomics: a row's values depend on its slots and the weights alone, not on the tile or the batch it is evaluated in.
 * Same library, status codes and enums as htf_amd.h; every pointer is a device pointer.
 */
#ifndef HTF_CFWIDE16_H_
#define HTF_CFWIDE16_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HTF_CFW16_MAX_H 256u
/* dynamic LDS of a launch: 256 (D32 + H1_32 + H2_32 + 24) + 4 (4 H2_32 + K4 + 68) bytes, widths rounded up to multiples of 32 and
 * K to a multiple of 4; 158 224 bytes at the limits.  Above this the call returns HTF_ERR_INVALID and launches nothing. */
#define HTF_CFW16_MAX_LDS_BYTES (160u * 1024u)

/* Argument for argument htf_cfw_grad (htf_cfwide.h): d_g [B][D] and d_energy [B] fp32 are written for the rows listed (d_rows,
 * n_rows; NULL: rows 0 .. n_rows - 1), one launch per species present.  d_weights: one network, Keras order, unpadded, fp32.
 * B = 0 or n_rows = 0 launches nothing. */
HTF_API int htf_cfw16_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types, unsigned H1,
                           unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap, float *d_g,
                           float *d_energy, const int *d_rows, unsigned n_rows, float r_cut, htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_CFWIDE16_H_ */
