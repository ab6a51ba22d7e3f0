/* htf_cforce.h -- conservative forces of the descriptor network (htf.DescriptorMLP(conservative=True)): F = -d(sum_i E_i)/dr
 * in two sweeps over the pair vectors, and the slot-aligned index tensor they need.
 *
 * htf_bp_forces (htf_bp.h) differentiates E_i with respect to row i's own pair vectors only.  E_j also depends on r_i
 * through G_j; with g_i = dE_i/dG_i (D floats per row) the force of the total energy is
 *
 *   phi_is = [ fc(r) c_der sum_k (g_i[t_j K + k] + g_j[t_i K + k]) (r - mu_k) e_k(r)
 *            + fc'(r)      sum_k (g_i[t_j K + k] + g_j[t_i K + k]) e_k(r) ] (x_ij + 1e-7) / r
 *   F_i    = sum_s live_is phi_is
 *   W_i    = -1/2 sum_s live_is x_ij (outer) phi_is
 *
 * with j = idx[i, s], r = r_ij, e_k(r) = exp(-(r - mu_k)^2 / gap), c_der = -2 / gap, and x_ij, r_ij, live, t_j, fc and fc'
 * exactly those of htf_bp.h (live also needs r < r_cut; no cutoff: fc = 1, fc' = 0); no factor 2.  t_i is row i's own type:
 * rint(d_types[i]), 0 for n_types = 1.  A neighbor type t_j outside [0, n_types) contributes nothing to G_i, so that slot's
 * g_i term is zero; its g_j term stays, because E_j still depends on r_i.
 *
 * The reverse term g_j is evaluated at row i's own r_ij and direction.  r_ji differs from it by the 1e-7 of safe_norm only,
 * which is below fp32 rounding at any distance a live slot has.  A slot whose index is outside [0, B), or any slot of a row
 * whose own type is outside [0, n_types), has no reverse term: nothing is read out of bounds, and such a row contributes to
 * nobody.
 *
 * F equals -d(sum_i E_i)/dr when the list is symmetric within the descriptor's range: full lists (j in row i whenever i
 * is in row j), no overflow of NN, and r_cut not above the cutoff of the list.  This is not checked.
 *
 * Pass 1 (htf_cf_grad) runs the rows of htf_bp_forces through the network's backward and writes g and E; pass 2
 * (htf_cf_forces) gathers K floats of g per slot.  Neither uses atomics: a row's bits depend on its slots, its indices and
 * the gathered rows of g alone, and E_i is bit for bit htf_bp_forces' energy.  Same library, status codes and enums as
 * htf_amd.h; every pointer is a device pointer.
 */
#ifndef HTF_CFORCE_H_
#define HTF_CFORCE_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Pass 1.  d_g [B][D] fp32 receives g_i = dE_i/dG_i and d_energy [B] fp32 E_i, for the rows listed (d_rows, n_rows and
 * d_weights as in htf_bp_forces: one launch per species present).  B = 0 or n_rows = 0 launches nothing. */
HTF_API int htf_cf_grad(const void *d_nlist, int nlist_dtype, unsigned B, unsigned NN, unsigned K, unsigned n_types, unsigned H1,
                        unsigned H2, int activation, const float *d_weights, const float *d_mu, float gap, float *d_g,
                        float *d_energy, const int *d_rows, unsigned n_rows, float r_cut, htf_stream stream);

/* Pass 2, every row in one launch.  d_index [B][NN] int32: the particle in each slot (any value on a slot that is not live).
 * d_types [B] fp32: the rows' own types, NULL for n_types = 1.  d_g, d_energy: what pass 1 wrote for every row.
 * d_force [B][4] (force_dtype): (F_i, E_i).  d_virial9, if not NULL, [B][9] (force_dtype): W_i, row-major. */
HTF_API int htf_cf_forces(const void *d_nlist, int nlist_dtype, const int *d_index, const float *d_types, unsigned B, unsigned NN,
                          unsigned K, unsigned n_types, const float *d_mu, float gap, const float *d_g, const float *d_energy,
                          void *d_force, int force_dtype, void *d_virial9, float r_cut, htf_stream stream);

/* The index tensor that goes with htf_build_pair_vectors on the same arguments: d_index [batch_size][NN] int32, slot s of row
 * w holds the particle whose pair vector htf_build_pair_vectors puts in slot s of row w, -1 for a zero-filled slot.  Rows
 * that overflow NN wrap like the pair vectors (entry q in slot q % NN, the last writer wins).  Positions fp32 or fp64. */
HTF_API int htf_cf_pair_index(int *d_index, const void *d_pos, int pos_dtype, unsigned N, unsigned NN, unsigned offset,
                              unsigned batch_size, const htf_box *box, const unsigned *d_n_neigh, const unsigned *d_nlist,
                              const unsigned *d_head_list, double rmax, htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_CFORCE_H_ */
