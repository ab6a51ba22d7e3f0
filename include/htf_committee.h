/* htf_committee.h -- a committee of descriptor networks (htf.DescriptorMLP(conservative=True, n_models=M)): the mean-model
 * conservative forces and the per-particle model deviation of M networks of one architecture, in the two sweeps of
 * htf_cforce.h.
 *
 * Member m, 0 <= m < M, 2 <= M <= 8, is the network of htf_cforce.h with its own weights: E_i^m, F_i^m = -d(sum_j E_j^m)/dr_i
 * and W_i^m are exactly that header's quantities for member m's weights -- the same slots, live, types, cutoff, reverse-term
 * rules, and no factor 2.  Per row i the committee gives
 *
 *   Ebar_i = (1/M) sum_m E_i^m        Fbar_i = (1/M) sum_m F_i^m        Wbar_i = (1/M) sum_m W_i^m
 *   devF_i = sqrt( (1/M) sum_m |F_i^m - Fbar_i|^2 )
 *   devE_i = sqrt( (1/M) sum_m (E_i^m - Ebar_i)^2 )
 *
 * The deviations take the population form and are computed as written, the mean first and then the differences, on the fp32
 * values of F_i^m and E_i^m: members that agree bit for bit have deviation 0, where the form <x^2> - <x>^2 would keep half
 * the digits.  The means are pairwise sums over the members divided by M: within 2^-22 max_m |F_i^m| of the exact mean of the
 * fp32 members.
 *
 * Nothing but the dense stack depends on the weights.  Pass 1 (htf_cmt_grad) reads a row's slots once, forms G_i once and runs
 * the M networks forward and backward on it; pass 2 (htf_cmt_forces) evaluates each exponential e_k(r) once per slot and centre
 * for all M members and gathers, per slot, the members' runs of one M D-float record of the table.  Neither uses atomics: a
 * row's bits depend on its slots, its indices and the gathered records alone.  Same library, status codes and enums as
 * htf_amd.h; every pointer is a device pointer.
 */
#ifndef HTF_COMMITTEE_H_
#define HTF_COMMITTEE_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HTF_CMT_MAX_MODELS 8
/* dynamic LDS a pass-1 launch may ask for (one workgroup owns the CU's LDS) */
#define HTF_CMT_MAX_LDS_BYTES (160u * 1024u)

/* Pass 1.  d_g [B][M][D] fp32 receives g_i^m = dE_i^m/dG_i, D = K n_types, and d_energy [B][M] fp32 E_i^m, for the rows listed
 * (d_rows, n_rows as in htf_cf_grad: one launch per species present).  Member m's weights are the P floats at
 * d_weights + m * weight_stride (the layout of htf_bp_forces); weight_stride >= P, in floats.  All M networks are staged in LDS
 * once per block of 16 waves: 4 * (M * P4 + K4 + 1024) bytes, P4 and K4 being P' = D (H1 + 1) + H1 (H2 + 1) + H1 + 2 H2 + 1 (rows padded
 * by one float) and K rounded up to multiples of 4.  Above HTF_CMT_MAX_LDS_BYTES the call returns HTF_ERR_INVALID and launches
 * nothing.  B = 0 or n_rows = 0 launches nothing. */
HTF_API int htf_cmt_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types, unsigned H1,
                         unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap, float *d_g,
                         float *d_energy, const int *d_rows, unsigned n_rows, float r_cut, unsigned n_models,
                         unsigned weight_stride, htf_stream stream);

/* Pass 2, every row in one launch.  d_index, d_types as in htf_cf_forces; d_g, d_energy: what pass 1 wrote for every row.
 * d_force [B][4] (force_dtype): (Fbar_i, Ebar_i).  d_virial9, if not NULL, [B][9] (force_dtype): Wbar_i, row-major.
 * d_dev [B][2] fp32: (devF_i, devE_i).  d_members, if not NULL, [M][B][4] fp32: (F_i^m, E_i^m). */
HTF_API int htf_cmt_forces(const void *d_nlist, int nlist_dtype, const int *d_index, const float *d_types, unsigned B, unsigned NN,
                           unsigned K, unsigned n_types, const float *d_mu, float gap, const float *d_g, const float *d_energy,
                           void *d_force, int force_dtype, void *d_virial9, float r_cut, unsigned n_models, float *d_dev,
                           float *d_members, htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_COMMITTEE_H_ */
