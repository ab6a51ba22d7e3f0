/* htf_cfw3train.h -- force matching on the conservative forces for networks with three hidden layers up to 256 wide
 * (htf.DescriptorMLP(trainable="deep", H3=...), DescriptorMLP.deep_loss_gradient): htf_cfw_loss_grad's sweep (htf_cfwtrain.h)
 * one layer deeper, as htf_cfw3_grad (htf_cfwide3.h) is htf_cfw_grad's.
 *
 * The quantity is htf_ctrain.h's, symbol for symbol: with the residual rho [B][4] held fixed,
 *
 *   SSR = sum_i |rho_i|^2 + rho_iE^2,    d SSR / d theta = 2 sum_i d( g_i . Gdot_i + rho_iE E_i ) / d theta
 *
 * over the listed rows, Gdot_i gathered from the neighbors' residuals through d_index, for
 * E_i = W4^T act(W3^T act(W2^T act(W1^T G_i + b1) + b2) + b3) + b4.  A tile of rows at a time: the rows' G and Gdot by the row
 * sweep's own sums, one forward pass that carries (value | tangent) through the three hidden layers and one reverse pass, every
 * product on v_mfma_f32_32x32x2_f32 in exact fp32; the gradients of W1, W2 and W3 are outer products of the tile's LDS images.
 * Each block adds its tiles into a partial [1 + P] of its own in d_scratch with plain loads and stores, and the partials are
 * added in a fixed order by the reduction htf_bp_loss_grad ends in.  No atomics; the grid and every order of summation are
 * functions of n_rows and the shapes alone, so two calls on the same inputs give the same bits.  Same library, status codes and
 * enums as htf_amd.h; every pointer is a device pointer.
 *
 * LDS.  A tile of R rows keeps four images, one line of 2 R floats per feature -- columns 0 .. R - 1 the VALUE of the rows,
 * columns R .. 2 R - 1 the TANGENT -- lines 2 R + 1 floats apart:
 *
 *   X [D32]  (G | Gdot)     A1 [H1_32]  (h1 | hd1), then (zb1 | zdb1)     A2 [H2_32]  (h2 | hd2), then (zb2 | zdb2)
 *   A3 [H3_32]  (zb3 | zdb3)
 *
 * (widths rounded up to multiples of 32; X is read again for dW1 at the very end, so no image shares its lines), and beside
 * them the centres, the tile's rho_E and the waves' scalars:
 *
 *   bytes(R) = 4 ((2 R + 1) (D32 + H1_32 + H2_32 + H3_32) + K4 + R + 16)        K4: K rounded up to 4
 *
 * The rule: R = 32 while bytes(32) <= HTF_CFW3_MAX_LDS_BYTES (at most 608 image lines), else R = 16.  At R = 16 a line is 33
 * floats and its 16 value and 16 tangent columns are the 32 columns of ONE matrix instruction, so a weight read still feeds
 * value and tangent.  With K = 16: bytes(32) is 33 536 at 16 x 32 x 32 x 32, 58 496 at 16 x 64 x 64 x 64, 108 416 at
 * 16 x 128^3 and 116 736 at 64 x 160 x 128 x 96 (108 416 at D = 16); 64 x 240^3 and 64 x 256^3 would need 216 576 there and
 * take 110 016 at R = 16 (110 208 with K = 64, the largest of all).  Every width triple in [1, 256]^3 with D <= 64 launches.
 */
#ifndef HTF_CFW3TRAIN_H_
#define HTF_CFW3TRAIN_H_
#include <stddef.h>
#include "htf_amd.h"
#include "htf_cfwide3.h"
#ifdef __cplusplus
extern "C" {
#endif

/* blocks of a launch at most: one per compute unit (the images of the wide shapes leave room for one block a unit); each owns
 * one partial */
#define HTF_CFW3T_MAX_BLOCKS 256u

/* floats of d_scratch for a launch over n_rows rows: min(ceil(n_rows / R), 256) (1 + P), R by the rule above and
 * P = D H1 + H1 + H1 H2 + H2 + H2 H3 + H3 + H3 + 1; 0 for n_rows = 0 and for shapes the sweep refuses.  The cap stays at one
 * block per compute unit: 152 MB at 64 x 256^3 (P = 148 481) and 4 096 rows or more, 45 MB at 64 x 160 x 128 x 96 and 8 192
 * rows or more -- half the blocks would halve the scratch and the sweep's rate with it. */
HTF_API size_t htf_cfw3_scratch_floats(unsigned n_rows, unsigned K, unsigned n_types, unsigned H1, unsigned H2, unsigned H3);

/* Argument for argument htf_cfw_loss_grad (htf_cfwtrain.h) with H3 after H2, 1 <= H1, H2, H3 <= HTF_CFW3_MAX_H: d_weights one
 * network in Keras order (W1, b1, W2, b2, W3, b3, W4, b4), d_index [B][NN] int32, d_rho [B][4] fp32 the residual of EVERY row,
 * d_accum [1 + P] OVERWRITTEN with {SSR, d SSR / d theta} in the order of the flat weights, d_scratch at least
 * htf_cfw3_scratch_floats(n_rows, ...) floats, d_rows / n_rows the species' row list (NULL: rows 0 .. n_rows - 1).  An index
 * outside [0, B) has no reverse term and nothing is read for it.  n_rows = 0: no sweep, d_accum receives zeros; B = 0: d_accum
 * may be NULL, and then nothing is launched.  Limits: K * n_types <= 64, NN <= 256. */
HTF_API int htf_cfw3_loss_grad(const void *d_nlist, int nlist_dtype, const int *d_index, unsigned B, unsigned NN, unsigned K,
                               unsigned n_types, unsigned H1, unsigned H2, unsigned H3, int activation, const float *d_weights,
                               const float *d_mu, float gap, const float *d_rho, float *d_accum, float *d_scratch,
                               const int *d_rows, unsigned n_rows, float r_cut, htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_CFW3TRAIN_H_ */
