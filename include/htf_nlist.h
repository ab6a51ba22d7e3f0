/* htf_nlist.h -- the cell-binned route of compute_nlist (utils.compute_nlist of hoomd-tf) on the device.
 *
 * The same neighbor list as htf_cg_nlist_forward (htf_cg.h), bit for bit, found by binning the particles into an
 * nx x ny x nz grid of cells over the orthorhombic box d_box_L = [Lx, Ly, Lz] and searching each row's 27 neighboring
 * cells instead of all M particles.  Same library (libhtf_amd.so), same status codes (htf_amd.h), fp32 arrays, every
 * pointer a device pointer unless stated.  The backward pass is htf_cg_nlist_backward: it works from d_idx alone.
 *
 * Exactness: every distance is measured as htf_cg_nlist_forward measures it, on the raw positions; the grid only chooses
 * which candidates a row looks at.  The caller picks nx, ny, nz >= 3 with L_c / n_c >= r_cut + 2^-14 (L_c + r_cut) per
 * dimension (hoomd_tf_amd/cgmap.py); the margin covers the fp32 rounding of the minimum image, so every pair at d <= r_cut
 * lies in neighboring cells.  A particle with a coordinate that is not finite or lies more than 64 box lengths from the
 * origin is binned into one extra cell that every row also searches, and its own row searches all M particles.
 */
#ifndef HTF_NLIST_H_
#define HTF_NLIST_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Words (4 bytes) of scratch htf_nlist_cells_forward needs for M particles and ncell = nx * ny * nz cells. */
HTF_API unsigned long long htf_nlist_cells_scratch_words(unsigned M, unsigned ncell);

/* The neighbor list of htf_cg_nlist_forward (same arguments, same d_out / d_idx) by the cell-binned search.
 * nx, ny, nz >= 3 (see above); d_scratch: htf_nlist_cells_scratch_words(M, nx * ny * nz) words, 16-byte aligned; the
 * call overwrites it.  Deterministic: two calls give the same bits. */
HTF_API int htf_nlist_cells_forward(const float *d_pos, unsigned pos_stride, unsigned M, const float *d_box_L, float r_cut,
                                    unsigned nx, unsigned ny, unsigned nz, unsigned NN, int sorted, int return_types,
                                    const unsigned char *d_excl, unsigned *d_scratch, float *d_out, int *d_idx,
                                    htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_NLIST_H_ */
