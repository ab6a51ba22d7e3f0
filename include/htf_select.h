/* htf_select.h -- frame selection by committee deviation on the device (htf.DeviationSelector): the consumer of the per-particle
 * model deviation that htf_cmt_forces leaves in d_dev [N][2] = (devF_i, devE_i).  One update classifies the current frame by its
 * largest deviation and, when the frame is worth labelling, keeps its positions and box in a buffer of `capacity` frames -- three
 * launches on the caller's stream, no read-back, nothing the host waits for.
 *
 * One update.  d_i = d_dev[2 i + column], 0 <= i < N (column 0: the force deviation, 1: the energy deviation).
 *
 *   a = the lowest i with d_i NaN, if any d_i is NaN; otherwise the lowest i with d_i >= d_j for every j
 *   s = d_a                             (so s = max_i d_i, and s is NaN exactly when some d_i is)
 *
 * -0 and +0 compare equal, as everywhere in IEEE arithmetic: among zeros of either sign the lowest index wins and s has its sign.
 * The pair (s, a) is the greatest element of a total order on (value, index) -- NaN above every number, larger values above
 * smaller ones, lower indices above higher ones at equal values -- and taking the greater of two pairs is associative and
 * commutative and rounds nothing.  So (s, a) does not depend on the grid, on max_blocks or on the order in which lanes, waves and
 * blocks are combined: every launch shape gives the same bits, and the tests compare with a sequential reference exactly.
 *
 * Classes (the DP-GEN rule), with 0 <= lo <= hi, lo finite, hi possibly +inf, both taken as fp32 like the deviations:
 *
 *   accurate    s <  lo
 *   candidate   lo <= s < hi
 *   failed      s >= hi, or s is NaN
 *
 * hi = +inf means that there is no upper threshold: no number fails, and s = +inf is a candidate then (the one case in which
 * the table's "s < hi" is not taken literally).  A NaN fails whatever hi is.
 *
 * Only a candidate may be stored.  While fewer than `capacity` frames are stored it takes the next free slot, slot = stored.
 * With the buffer full:
 *   HTF_SEL_FIRST    the frame is dropped;
 *   HTF_SEL_LARGEST  let j be the lowest slot holding the smallest stored s.  The frame replaces slot j if its own s is strictly
 *                    larger than that; otherwise (an equal s included) it is dropped.
 * A stored frame is the N rows of d_pos [N][4], the nine values of d_box [3][3] (zeros when d_box is NULL), s, a and stamp, the
 * 0-based ordinal of the update since the last reset.
 *
 * Counters (32-bit, wrapping): seen = accurate + candidate + failed; candidate = stored + replaced + dropped; stored <= capacity
 * is the number of occupied slots, which are slots [0, stored).
 *
 * State.  d_state is htf_sel_state_words(capacity) 32-bit words owned by the caller; all zeros is the empty selector (what
 * htf_sel_reset writes).  Word HTF_SEL_SEEN .. HTF_SEL_REPLACED: the counters.  HTF_SEL_SLOT (int): the slot the last update
 * stored to, or -1.  HTF_SEL_LAST, HTF_SEL_LAST + 1 (float): s and (float)a of the last update.  From HTF_SEL_HEADER_WORDS:
 * float s[capacity], unsigned a[capacity], unsigned stamp[capacity]; then the reduction's partials, 2 HTF_SEL_MAX_BLOCKS words.
 *
 * Same library, status codes and dtype enums as htf_amd.h; every pointer is a device pointer.  Every argument check precedes
 * the first HIP call: a refused call returns HTF_ERR_INVALID and launches nothing.
 */
#ifndef HTF_SELECT_H_
#define HTF_SELECT_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HTF_SEL_MAX_CAPACITY 65536u
/* the most blocks the reduction runs, and the default cap (max_blocks = 0): four blocks of 256 rows per compute unit */
#define HTF_SEL_MAX_BLOCKS 1024u

enum { HTF_SEL_FIRST = 0, HTF_SEL_LARGEST = 1 };
enum { HTF_SEL_FORCE = 0, HTF_SEL_ENERGY = 1 };
enum {
    HTF_SEL_SEEN = 0, HTF_SEL_ACCURATE = 1, HTF_SEL_CANDIDATE = 2, HTF_SEL_FAILED = 3, HTF_SEL_STORED = 4, HTF_SEL_DROPPED = 5,
    HTF_SEL_REPLACED = 6, HTF_SEL_SLOT = 7, HTF_SEL_LAST = 8, HTF_SEL_HEADER_WORDS = 16
};

/* 32-bit words of the state for a buffer of `capacity` frames; 0 when capacity is outside [1, HTF_SEL_MAX_CAPACITY]. */
HTF_API unsigned long long htf_sel_state_words(unsigned capacity);

/* One update, at most three launches on `stream`:
 *   reduce   min(ceil(N / 256), max_blocks) blocks of 256 stride over the column and leave one (value, index) pair each;
 *            max_blocks = 0 means HTF_SEL_MAX_BLOCKS, and a value above that is refused;
 *   decide   one block: (s, a) of the partials, the class, the counters, the slot (for HTF_SEL_LARGEST a scan of the stored s)
 *            and, when the frame is stored, the slot's (s, a, stamp);
 *   store    copies d_pos to d_frames[slot] and d_box to d_boxes[slot]; every block reads the slot word and returns at -1.
 * d_pos [N][4] and d_box [3][3] (or NULL) hold `dtype` (HTF_F32 or HTF_F64), and so do d_frames [capacity][N][4] and d_boxes
 * [capacity][9]: rows are copied, never converted.  d_pos and d_frames are 16-byte aligned.  N >= 1. */
HTF_API int htf_sel_update(const float *d_dev, unsigned N, int column, float lo, float hi, int policy, unsigned capacity,
                           unsigned *d_state, const void *d_pos, const void *d_box, int dtype, void *d_frames, void *d_boxes,
                           unsigned max_blocks, htf_stream stream);

/* Empties the selector on `stream`: the whole state to zero (one memset node; the frame buffers keep their bytes, which no slot
 * names any more). */
HTF_API int htf_sel_reset(unsigned *d_state, unsigned capacity, htf_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HTF_SELECT_H_ */
