/* htf_step_check.h -- the check step of the stand-in's device-decided neighbor list WITHOUT a check launch.  Part of htf_standin.h
 * (which includes it, behind htfs_nlist) and, like it, outside the drop-in boundary.
 * With an odd check period the step before a check is a classic step: force launch, integrator launch.  The integrator has every
 * new position in a register when it stores it, so it can leave the check's displacement word behind; the check is then the gated
 * rebuild launches alone, and its two status words can ride to the host on the force launch that follows (htfs_step_epilogue's
 * d_mail_src / h_mail_dst) instead of in a copy of their own. */
#ifndef HTF_STEP_CHECK_H_
#define HTF_STEP_CHECK_H_
#include "htf_standin.h"
#ifdef __cplusplus
extern "C" {
#endif

/* htfs_nve_step and the distance check of the NEXT step in one launch: the same update and stores, and *d_disp2 <- the word
 * htfs_max_displacement2 would give on the stored positions (from nl->ref, on nl->box; same bits), accumulated in the two work words
 * of nl->scratch -- zero before the call, zero after it.  The integrator has every new position in a register when it stores it: a
 * check step that follows needs no sweep of its own, only htfs_rebuild_nlist_gated.  1024 rows per workgroup. */
HTF_API int htfs_nve_step_check(void *d_pos, void *d_vel, const void *d_force, int dtype, unsigned N,
                                double dt, const htf_box *box, const htfs_nlist *nl, float *d_disp2, htf_stream stream);

/* The same check step behind a displacement word that is ALREADY in *d_disp2 (htfs_nve_step_check left it there): the five gated
 * launches and nothing before them.  The copy of the status words is issued only when h_stat2 != NULL and !h_stat2_by_mail -- by
 * mail: the force launch behind this call carries them to the host (htfs_step_epilogue's d_mail_src / h_mail_dst). */
HTF_API int htfs_rebuild_nlist_gated(const htfs_nlist *nl, const void *d_pos, int dtype, unsigned N, unsigned Ntot, int scratch_clean,
                                     float *d_disp2, double threshold2, unsigned *d_stat2, unsigned *h_stat2, int h_stat2_by_mail,
                                     htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif
