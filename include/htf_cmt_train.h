/* htf_cmt_train.h -- force matching for every member of a committee of descriptor networks in one sweep
 * (htf.DescriptorMLP(n_models=M, trainable="committee"), DescriptorMLP.committee_loss_gradient).
 *
 * Member m, 0 <= m < M, 2 <= M <= HTF_CMT_MAX_MODELS (htf_committee.h), is fitted on its own against the same labels: the
 * committee's loss is sum_m SSR^m and no term couples two members.  With the residual of every particle held fixed,
 *
 *   rho_i^m  = (F_i^m - F_i^label, E_i^m - E_i^label)           d_rho [B][M][4] fp32, (F_i^m, E_i^m) as htf_cmt_forces' d_members
 *   accum[m] = {SSR^m, d SSR^m / d theta^m}                      [1 + P] floats at d_accum + m * accum_stride
 *
 * are exactly htf_ct_loss_grad's quantities (htf_ctrain.h) for member m's weights and d_rho = rho^m: the same Gdot, R'_k, u_is,
 * m_is and live, the same cutoff terms, no factor 2 inside Gdot, rho held fixed, rows listed per species, and an index outside
 * [0, B) contributes no reverse term.
 *
 * What a row reads does not depend on the member: the pair vectors [B][NN][4], the index [B][NN] and, per live slot, the
 * neighbor's residual.  A block runs one wave per member and its waves walk the same rows in the same order, so those reads
 * come from HBM once per row and from the caches for the other M - 1 waves (every wave issues them); the residual of a particle
 * is one 16 M-byte record of which wave m gathers its own float4.  Nor do e_k(r) and R'_k(r) depend on the member: the block's
 * waves split the K centres, each forms the exponentials of its centres once, G once and Gdot^m for every member from the
 * a^m = ((rho_i^m - m_is rho_j^m) . u_is) the waves publish in LDS (two block barriers per row).  Each wave keeps member m's
 * network in LDS (all M are staged once per block), its own exchange lines and its own gradient accumulators in registers,
 * runs the network passes of its member and writes its member's block partial itself; the
 * partials of all members are added in a fixed order by one launch of a second instance of the library's reduction.  No atomics
 * and no memset; the grid is a function of n_rows and M alone.
 *
 * Bit contracts: (a) two calls on the same inputs give the same bits; (b) member m's [1 + P] depends on member m's weights and
 * residuals alone, and on no other member's.  Same library, status codes and enums as htf_amd.h; every pointer is a device
 * pointer.
 */
#ifndef HTF_CMT_TRAIN_H_
#define HTF_CMT_TRAIN_H_
#include "htf_amd.h"
#include "htf_committee.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Floats of d_scratch for a call on n_rows rows: one partial [1 + P] per block and member.  0 for limits the sweep refuses. */
HTF_API size_t htf_cmt_scratch_floats(unsigned n_rows, unsigned K, unsigned n_types, unsigned H1, unsigned H2, unsigned n_models);

/* d_nlist, d_index, d_mu, gap, d_rows, n_rows, r_cut and the limits as in htf_ct_loss_grad.  Member m's weights are the P floats
 * at d_weights + m * weight_stride (weight_stride >= P, in floats, as in htf_cmt_grad).  d_rho [B][M][4] fp32: the residual of
 * EVERY row, listed or not.  Member m's {SSR^m, d SSR^m / d theta^m} goes to d_accum + m * accum_stride (accum_stride >= 1 + P)
 * and is OVERWRITTEN (n_rows = 0: the sweep is not launched and the M results are zeros; B = 0: d_accum may be NULL, and then
 * nothing is launched).  d_scratch: at least htf_cmt_scratch_floats(n_rows, ...) floats.  The launch keeps all M networks and
 * six exchange lines and 256 slot terms per member in LDS: 4 * (M * (P4 + 640) + K4) bytes, P4 and K4 as in htf_cmt_grad.  Above
 * HTF_CMT_MAX_LDS_BYTES the call returns HTF_ERR_INVALID, launches nothing and leaves both byte counts in htf_last_error(). */
HTF_API int htf_cmt_loss_grad(const void *d_nlist, int nlist_dtype, const int *d_index, unsigned B, unsigned NN, unsigned K,
                              unsigned n_types, unsigned H1, unsigned H2, int activation, const float *d_weights, const float *d_mu,
                              float gap, const float *d_rho, float *d_accum, float *d_scratch, const int *d_rows, unsigned n_rows,
                              float r_cut, unsigned n_models, unsigned weight_stride, unsigned accum_stride, htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_CMT_TRAIN_H_ */
