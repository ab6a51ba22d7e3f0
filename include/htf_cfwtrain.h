/* htf_cfwtrain.h -- force matching on the conservative forces for networks with hidden layers up to 256 wide
 * (htf.DescriptorMLP(trainable="wide"), DescriptorMLP.wide_loss_gradient): htf_ct_loss_grad's sweep (htf_ctrain.h) with the
 * dense stack on the fp32 matrix instruction, as htf_cfw_grad (htf_cfwide.h) is htf_cf_grad's.
 *
 * The quantity is htf_ctrain.h's, symbol for symbol: with the residual rho [B][4] held fixed,
 *
 *   SSR = sum_i |rho_i|^2 + rho_iE^2,    d SSR / d theta = 2 sum_i d( g_i . Gdot_i + rho_iE E_i ) / d theta
 *
 * over the listed rows, Gdot_i gathered from the neighbors' residuals through d_index.  A tile of 32 rows at a time: the rows'
 * G and Gdot by the row sweep's own sums, then one forward pass that carries (value | tangent) through both hidden layers and
 * one reverse pass, every product on v_mfma_f32_32x32x2_f32 in exact fp32; the weight gradients of the two matrices are outer
 * products of the tile's LDS images.  Each block adds its tiles into a partial [1 + P] of its own in d_scratch with plain loads
 * and stores, and the partials are added in a fixed order by the reduction htf_bp_loss_grad ends in.  No atomics; the grid and
 * every order of summation are functions of n_rows and the shapes alone, so two calls on the same inputs give the same bits.
 * The result agrees with htf_ct_loss_grad's to rounding, not bit for bit.  Same library, status codes and enums as htf_amd.h;
 * every pointer is a device pointer.
 */
#ifndef HTF_CFWTRAIN_H_
#define HTF_CFWTRAIN_H_
#include <stddef.h>
#include "htf_amd.h"
#include "htf_cfwide.h"
#ifdef __cplusplus
extern "C" {
#endif

/* blocks of a launch at most: one per compute unit; each owns one partial */
#define HTF_CFWT_MAX_BLOCKS 256u
/* rows of a tile */
#define HTF_CFWT_TILE_ROWS 32u

/* floats of d_scratch for a launch over n_rows rows: min(ceil(n_rows / 32), 256) (1 + P); 0 for n_rows = 0 and for shapes
 * the sweep refuses.  85 MB at 64 x 256 x 256 and 8 192 rows or more. */
HTF_API size_t htf_cfw_scratch_floats(unsigned n_rows, unsigned K, unsigned n_types, unsigned H1, unsigned H2);

/* Argument for argument htf_ct_loss_grad (htf_ctrain.h), with 1 <= H1, H2 <= HTF_CFW_MAX_H: d_index [B][NN] int32, d_rho
 * [B][4] fp32 the residual of EVERY row, d_accum [1 + P] OVERWRITTEN with {SSR, d SSR / d theta} in the order of the flat
 * weights, d_scratch at least htf_cfw_scratch_floats(n_rows, ...) floats, d_rows / n_rows the species' row list (NULL: rows
 * 0 .. n_rows - 1).  An index outside [0, B) has no reverse term and nothing is read for it.  n_rows = 0: no sweep, d_accum
 * receives zeros; B = 0: d_accum may be NULL, and then nothing is launched.  Limits: K * n_types <= 64, NN <= 256, and the
 * LDS of htf_cfwide.h (HTF_CFW_MAX_LDS_BYTES). */
HTF_API int htf_cfw_loss_grad(const void *d_nlist, int nlist_dtype, const int *d_index, unsigned B, unsigned NN, unsigned K,
                              unsigned n_types, unsigned H1, unsigned H2, int activation, const float *d_weights, const float *d_mu,
                              float gap, const float *d_rho, float *d_accum, float *d_scratch, const int *d_rows, unsigned n_rows,
                              float r_cut, htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_CFWTRAIN_H_ */
