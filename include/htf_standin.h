/* htf_standin.h -- stand-in for the parts of HOOMD-blue that sit either side of the
 * force path (integrator, cell-list neighbor search) so that "MD steps/s" can be
 * measured without HOOMD.  NOT part of the drop-in boundary (that is htf_amd.h): a real
 * deployment keeps HOOMD's own integrator and NeighborList and never links this.
 * Arrays use HOOMD layouts (Scalar4 pos/vel/force; n_neigh/head_list/nlist, FULL mode).
 */
#ifndef HTF_STANDIN_H_
#define HTF_STANDIN_H_
#include "htf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Leapfrog form of velocity Verlet (unit mass): v += dt*f; x += dt*v; wrap into the
 * periodic box; pos.w (type bits) untouched.  IntegratorTwoStep + TwoStepNVE analogue. */
HTF_API int htfs_nve_step(void *d_pos, void *d_vel, const void *d_force, int dtype, unsigned N,
                          double dt, const htf_box *box, htf_stream stream);

/* *d_out (float, caller zeroes) = max_i |minimage(pos_i - ref_i)|^2: the neighbor list
 * must be rebuilt once this exceeds (r_buff/2)^2 (NeighborList::distanceCheck). */
HTF_API int htfs_max_displacement2(const void *d_pos, const void *d_ref, int dtype, unsigned N,
                                   const htf_box *box, float *d_out, htf_stream stream);

/* The same check for a replayed (hipGraph) cycle in ONE launch: d_work (2 words, zero before the first call and left zero by every
 * call) accumulates, the last workgroup publishes d_out[0] = the largest squared displacement and d_out[1] += 1 (the cycle number:
 * an UNSIGNED 32-bit word stored in the float slot's bits, compared modulo 2^32 by the host -- a float value stopped at 2^24).  h_out (nullable; PINNED host memory, device-accessible) receives the same two words, the cycle number last behind
 * a system-scope fence; `mirror` (nullable) lists up to HTFS_MIRROR_MAX word ranges the same workgroup copies from device to
 * pinned host memory BEFORE that -- status words earlier kernels left behind (htfs_brick counts, the list's largest row) -- so a
 * host that reads cycle c in h_out reads everything up to the end of cycle c - 1 beside it, without one copy node in the chain. */
#define HTFS_MIRROR_MAX 4
typedef struct htfs_mirror {
    const void *src[HTFS_MIRROR_MAX];
    void *dst[HTFS_MIRROR_MAX];
    unsigned words[HTFS_MIRROR_MAX];
    unsigned n;
} htfs_mirror;
HTF_API int htfs_check_displacement2(const void *d_pos, const void *d_ref, int dtype, unsigned N, const htf_box *box,
                                     unsigned *d_work, float *d_out, float *h_out, const htfs_mirror *mirror, htf_stream stream);

/* Cell-list neighbor search in HOOMD layout (NeighborListGPUBinned analogue): everything that describes a list between
 * rebuilds.  The caller owns every buffer; a hipGraph that has captured a rebuild carries these addresses by value.
 * The search walks the neighbor cells of each local particle -- stencil3[d] = 0 (one cell along d), 1 (cells at least r_list
 * wide, 3 per direction) or 2 (at least r_list / 2 wide, 5 per direction) -- in the cell-sorted copy and writes
 *   nlist[i*pitch + c] = k  for every k != i with |minimage(r_k - r_i)| <= r_list,
 *   n_neigh[i] = count, head_list[i] = i*pitch. */
#define HTFS_RANGE_WORDS(ncell, stencil_y, stencil_z) (4u * (size_t)(ncell) * (2u * (stencil_y) + 1u) * (2u * (stencil_z) + 1u))
/* htfs_nlist's scratch, in 32-bit words: counts | cursors | work words | staging (2 * ncell + 2 + Ntot; until the per-cell ordering
 * moved into the rebuild's finishing kernel it was 2 * ncell) */
#define HTFS_SCRATCH_WORK(ncell) (2u * (size_t)(ncell))
#define HTFS_SCRATCH_STAGE(ncell) (HTFS_SCRATCH_WORK(ncell) + 2u)
#define HTFS_SCRATCH_WORDS(ncell, Ntot) (HTFS_SCRATCH_STAGE(ncell) + (size_t)(Ntot))
typedef struct htfs_nlist {
    htf_box box;            /* the box the list is binned and searched on (a brick + its ghost layer under a local grid) */
    double r_list;
    int ncell3[3];          /* cells per direction, x fastest; ncell = their product */
    int stencil3[3];
    unsigned pitch;
    int type_split;         /* >= 0: pairs whose types lie on different sides of it are left out (hoomd.md.nlist.rcut
                             * set_pair(..., -1) between all-atom and mapped bead types, tensorflowcompute.py:284-305); -1: no filter */
    /* scratch of a rebuild, Ntot = local rows + ghosts */
    unsigned *cell_of;      /* [Ntot] cell index of every particle; 0xFFFFFFFF for an INERT row (x = NaN: fixed-capacity arrays of
                             * a decomposed system, hoomd_tf_amd/brick.py -- such rows are in no cell) */
    unsigned *scratch;      /* [HTFS_SCRATCH_WORDS(ncell, Ntot)], 16-byte aligned (checked): the per-cell counts [ncell], the scatter's
                             * cursors [ncell], the two work words of htfs_check_rebuild_nlist's distance check, and [Ntot] staging
                             * words (every cell's members in the order the scatter's atomics left them, before the rebuild ranks
                             * them into `order`).  The counts and the work words are zero after every COMPLETED call on it with the
                             * same ncell, as long as nothing else has written the buffer: that is what a caller passing
                             * scratch_clean != 0 promises, and the call then skips its memsets (dependent nodes of a captured
                             * rebuild; a rebuild a closed gate holds back does not touch the counts either).  htfs_cell_sort uses
                             * the first 2 * ncell words of the same buffer and keeps the promise */
    unsigned *cell_start;   /* [ncell + 1] first slot of cell c; the last word is the binned total */
    unsigned *order;        /* [Ntot] particle indices sorted by cell, ascending index inside a cell (deterministic) */
    void *pos_sorted;       /* [Ntot] Scalar4 pos[order] with  order[i] | (type >= type_split) << 31  in w (Ntot <= 2^31): a cell's
                             * members are contiguous and one load brings a candidate's position and identity */
    void *ranges;           /* HTFS_RANGE_WORDS(ncell, stencil3[1], stencil3[2]) words, 16-byte aligned: the candidate-range table.
                             * Every rebuild rewrites it before the search reads it */
    /* outputs */
    unsigned *n_neigh;      /* [N] */
    unsigned *head_list;    /* [N] */
    unsigned *nlist;        /* [N * pitch] */
    unsigned *max_neigh;    /* the largest count (> pitch: the list overflowed and must be rebuilt with a larger pitch); a
                             * rebuild a closed gate holds back leaves the previous value */
    void *ref;              /* nullable: [N] Scalar4 <- pos at a rebuild (what htfs_max_displacement2 measures from) */
    unsigned *counter;      /* nullable: += 1 at a rebuild */
    double image_L[3];      /* 0 = leave the axis alone.  Along an axis the grid is NOT periodic on, the period the caller's
                             * coordinates have -- the logical box length of a decomposed system -- so that a coordinate is binned,
                             * and copied into pos_sorted, as its image nearest the grid's centre (a row that left the brick through a
                             * face on the box boundary was wrapped to the far side by the integrator; the search measures plain
                             * differences along such an axis) */
} htfs_nlist;

/* The stepwise form, for a first build that sizes its buffers between the steps.  cell index of every particle: */
HTF_API int htfs_cell_index(const void *d_pos, int dtype, unsigned Ntot, const htf_box *box,
                            const int *ncell3, unsigned *d_cell_of, htf_stream stream);
/* counting sort by cell: htfs_nlist's order and cell_start from cell_of; d_scratch as htfs_nlist's, always zeroed first */
HTF_API int htfs_cell_sort(const unsigned *d_cell_of, unsigned Ntot, unsigned ncell, unsigned *d_scratch,
                           unsigned *d_cell_start, unsigned *d_order, htf_stream stream);
/* htfs_nlist's pos_sorted from pos and order */
HTF_API int htfs_gather4_tagged(void *d_dest, const void *d_src, const int *d_order, int dtype, unsigned n, int type_split,
                                htf_stream stream);
/* the same for arrays with inert rows: only the first *d_n_live entries of d_order exist, d_n_live = d_cell_start + ncell (the
 * binned total), read on the device */
HTF_API int htfs_gather4_tagged_live(void *d_dest, const void *d_src, const int *d_order, int dtype, unsigned n_max,
                                     const unsigned *d_n_live, int type_split, htf_stream stream);
/* range table + search of the N local rows of d_pos, on cell_start and pos_sorted as the calls above left them */
HTF_API int htfs_build_nlist(const htfs_nlist *nl, const void *d_pos, int dtype, unsigned N, htf_stream stream);

/* The whole rebuild in one call and five launches (the stepwise calls take ten): Ntot >= N positions binned, the N local rows
 * searched, ref and counter committed. */
HTF_API int htfs_rebuild_nlist(const htfs_nlist *nl, const void *d_pos, int dtype, unsigned N, unsigned Ntot, int scratch_clean,
                               htf_stream stream);

/* One check step of a device-decided list in one call, WITHOUT a host decision: *d_disp2 <- max_i |minimage(pos_i - ref_i)|^2
 * (from nl->ref, required; the value htfs_max_displacement2 gives, by one launch that accumulates in the scratch's work words
 * and needs no zeroing), then the rebuild above with every kernel returning at entry unless *d_disp2 > threshold2 when it
 * RUNS; the caller enqueues it behind every distance check and never reads the result back.  d_stat2 stands in for
 * nl->max_neigh and nl->counter (d_stat2[0] = largest row, d_stat2[1] = rebuilds); h_stat2 (nullable; pinned host memory)
 * receives an asynchronous copy of the two words, behind the search, for a later check to read.  Seven stream operations,
 * five of them gated. */
HTF_API int htfs_check_rebuild_nlist(const htfs_nlist *nl, const void *d_pos, int dtype, unsigned N, unsigned Ntot, int scratch_clean,
                                     float *d_disp2, double threshold2, unsigned *d_stat2, unsigned *h_stat2, htf_stream stream);

/* Slab decomposition (the stand-in for HOOMD's Communicator; hoomd_tf_amd/domain.py): the migration + ghost plan of a
 * rebuild.  d_key[i] = destination * 4 + ghost class of local particle i (destination: 0 stay, 1 left neighbor,
 * 2 right neighbor, 3 beyond; class in the slab it ends up in: 0 interior, 1 near the left face only, 2 near both,
 * 3 near the right face only).  d_bounds: world + 1 slab boundaries along x in the positions' dtype.  htfs_key_sort16 over
 * these keys then yields the stable (destination, class) order and the 16 counts. */
HTF_API int htfs_slab_classify(const void *d_pos, int dtype, unsigned N, const void *d_bounds, int world, int rank,
                               double r_ghost, unsigned *d_key, htf_stream stream);

/* Stable counting sort of N elements by a key < 16: d_order <- indices grouped by key, ascending index inside a key;
 * d_start[k] <- first slot of key k (17 entries).  d_scratch: 16 * ceil(N / 4096) words.  (htfs_cell_sort is the tool for
 * many cells of a few members; this one for a few keys of many members.) */
HTF_API int htfs_key_sort16(const unsigned *d_key, unsigned N, unsigned *d_scratch, unsigned *d_start, unsigned *d_order,
                            htf_stream stream);

/* dst[dst_start[s] + j] = src[src_start[s] + j] for j < count[s], s < n_segments <= HTFS_MAX_SEGMENTS, rows of
 * row_bytes (a multiple of 4): merges class-sorted segments into one class-sorted array in one launch. */
#define HTFS_MAX_SEGMENTS 16
HTF_API int htfs_segment_copy(void *d_dst, const void *d_src, unsigned row_bytes, unsigned n_segments,
                              const unsigned *src_start, const unsigned *dst_start, const unsigned *count, htf_stream stream);

/* ---- Brick decomposition with fixed-capacity arrays (round 5; hoomd_tf_amd/brick.py BrickDomain) --------------------------------
 * The stand-in for HOOMD's Communicator on a px x py (x 1) grid of ranks, built so that NOTHING a rebuild produces has to be read by
 * the host: local rows live in [0, cap_int) (particles with no ghost neighbor, then INERT rows) and [cap_int, cap_int + cap_bnd)
 * (particles within r_ghost of a face, ordered by class, then inert rows); ghosts of message m live in a fixed region of
 * ghost_cap[m] rows behind them.  An inert row has x = NaN (never a neighbor, in no cell, empty neighbor row, zero velocity), so
 * every launch is sized by a capacity and particle counts, message counts and class boundaries stay on the device (d_counts).
 * Messages are numbered by neighbor offset o in {-1, 0, +1}^ndim: index = sum_d (o_d + 1) 3^d with the centre skipped.
 * Class of a particle along a decomposed axis: 0 away from both faces, 1 within r_ghost of the low face only, 2 of both, 3 of the
 * high face only; class key = k_0 + 4 k_1; interior = key 0.  Message to offset o carries the rows whose class is near the low
 * (o_d = -1) / high (o_d = +1) face along every axis with o_d != 0, in row order.
 * Replica mode: one rank that is its own neighbor in every direction (a p-fold periodic replication of its brick): messages are
 * shifted by -o_d * width_d (shift[m]), so ghosts and returning migrants appear where a real neighbor's would. */
#define HTFS_BRICK_MAX_MSG 8
#define HTFS_BRICK_MAX_P 64
typedef struct htfs_brick {
    int ndim;                                   /* decomposed axes: 1 or 2 */
    int axis[2];                                /* box axis of each (0 x, 1 y, 2 z) */
    int p[2];                                   /* bricks along it */
    int me[2];                                  /* this rank's brick coordinate */
    int n_msg;                                  /* 3^ndim - 1 */
    int replica;                                /* this rank is its own neighbor in every direction (messages are shifted) */
    double r_ghost;
    unsigned cap_int, cap_bnd;
    unsigned ghost_cap[HTFS_BRICK_MAX_MSG];     /* rows of halo message m (sent AND received: capacities are symmetric) */
    unsigned ghost_off[HTFS_BRICK_MAX_MSG];     /* first row of message m in the packed send buffer; a message RECEIVED from the neighbor
                                                 * at offset o lands at ghost row ghost_off[index(o)] (source offsets ascending) */
    unsigned mig_cap[HTFS_BRICK_MAX_MSG];       /* rows of migration message m, its header row included */
    unsigned mig_off[HTFS_BRICK_MAX_MSG];       /* first row of message m in the migration send buffer / of the message from offset o
                                                 * in the receive buffer */
    double shift[HTFS_BRICK_MAX_MSG][3];        /* added to the positions HALO message m carries: replica mode -o_d * brick width; with a
                                                 * brick-local cell grid also the box vector of a message that crosses the periodic
                                                 * boundary (ghosts then sit next to the brick, as HOOMD wraps its ghosts) */
    double mig_shift[HTFS_BRICK_MAX_MSG][3];    /* the same for MIGRATION message m (replica mode only: a real migrant has already been
                                                 * wrapped into its new owner's brick by the integrator) */
    int halo_wrap, mig_wrap;                    /* wrap a shifted position back into the global box (halo: only when the list is binned
                                                 * on the global box's grid; migration: replica mode) */
    double box_lo[3], box_L[3];                 /* the global (in replica mode: logical) periodic box: a shifted position is wrapped
                                                 * back into it, as the integrator wraps (ghosts and migrants keep coordinates the
                                                 * cell list can bin; the pair-vector build takes the minimum image anyway) */
} htfs_brick;

/* device words of d_counts */
enum {
    HTFS_BC_N_INT = 0,      /* particles in the interior segment */
    HTFS_BC_N_BND = 1,      /* particles in the boundary segment */
    HTFS_BC_N_CAND = 2,     /* stayed + arrived at the last rebuild */
    HTFS_BC_N_ARRIVED = 3,  /* migrants received, cumulative */
    HTFS_BC_FLAGS = 4,      /* HTFS_BF_* bits, sticky until the caller clears them */
    HTFS_BC_REBUILDS = 5,
    HTFS_BC_MSG = 8,        /* [8, 16): rows of halo message m */
    HTFS_BC_CLASS = 16,     /* [16, 16 + 18): first candidate of class c in class order (c = 0..16), then the total */
    HTFS_BC_SLOT = 64,      /* [64, 64 + 16 * 8): first slot of class c in halo message m (word 64 + 8 c + m), 0xFFFFFFFF: not carried */
    HTFS_BC_WORDS = 192
};
enum {
    HTFS_BF_LOST = 1,           /* a particle crossed more than one brick between rebuilds */
    HTFS_BF_MIG_OVERFLOW = 2,   /* more migrants than a migration message holds */
    HTFS_BF_INT_OVERFLOW = 4,
    HTFS_BF_BND_OVERFLOW = 8,
    HTFS_BF_GHOST_OVERFLOW = 16,
    HTFS_BF_HALO_TIMEOUT = 32   /* transport "peer": a neighbor's message did not arrive within the spin limit */
};

/* A FLAGGED plan (tests/test_gpu_brick_kernels.py test_overflows): the kernels clamp and carry on, and store nothing outside their
 * arrays.  MIG_OVERFLOW: the header count is min(n, mig_cap[m] - 1), the first so many migrants of the message travel, the others
 * are in no message and no candidate list.  INT / BND_OVERFLOW: N_INT / N_BND are clamped to the capacity and the first cap_int /
 * cap_bnd rows of the class-sorted candidates are placed; CLASS[] and N_CAND keep the unclamped boundaries, so after a BND_OVERFLOW
 * the halo pack reads up to pos[cap_int + n_bnd - 1], past the local rows (the caller's array has the ghost region there).
 * GHOST_OVERFLOW: MSG[m] is clamped to ghost_cap[m], the message is its first ghost_cap[m] rows in class order, the rows cut off
 * have 0xFFFFFFFF in htfs_brick_row_slots.  LOST: the row's destination key is 0 -- it stays a candidate of this brick.
 * A rebuild writes N_INT, N_BND, N_CAND, MSG[0 .. n_msg), CLASS[0 .. 4^ndim] and all of SLOT, adds to N_ARRIVED and REBUILDS, ORs
 * into FLAGS, and leaves every other word of d_counts alone. */

/* scratch of a rebuild, all caller-owned: cand = cap_int + cap_bnd + sum_m mig_cap[m] candidate slots */
typedef struct htfs_brick_work {
    unsigned *key;          /* [cand] */
    unsigned *order;        /* [cand] */
    unsigned *sort_scratch; /* [32 * ceil(cand / 1024)] */
    unsigned *start1;       /* [17]  destination-key starts of the first sort */
    unsigned *start2;       /* [33]  class-key starts of the second */
    void *tmp_pos;          /* [cand] Scalar4 */
    void *tmp_vel;          /* [cand] Scalar4 */
} htfs_brick_work;

/* The halo WITHOUT a communication library (transport "peer", round 5): the packing kernels store every message row straight
 * into the RECEIVER's staging buffer -- its own memory for a replica rank, an IPC-mapped buffer of another process / device over xGMI
 * otherwise -- and the last workgroup to finish publishes, per message, the row count and the exchange's sequence number
 * (system-scope release); the receiver's htfs_brick_unpack_halo waits for the numbers of its incoming messages (acquire, bounded
 * spin) and copies the rows into the ghost region.  Everything is ordinary kernel work on ONE stream -- capturable into a hipGraph,
 * and the stores travel while the interior rows are evaluated.  Staging is double-buffered by the sequence number's parity: a
 * neighbor that is a step ahead writes the other half.  Every rank performs the same sequence of exchanges (lockstep counters). */
typedef struct htfs_peer {
    void *inbox[HTFS_BRICK_MAX_MSG];       /* message m's destination: the inbox of the neighbor at offset m, [2][ghost rows] Scalar4 */
    unsigned *signal[HTFS_BRICK_MAX_MSG];  /* ... and that neighbor's signal words, [2 * n_msg]: {sequence, rows} per source offset */
    void *my_inbox;                        /* this rank's own inbox and signal words (what htfs_brick_unpack_halo reads) */
    unsigned *my_signal;
    unsigned *state;                       /* this rank's [4]: exchanges done, workgroups finished, timeouts seen, spare */
    unsigned spin_limit;                   /* polls of a signal word before giving up (HTFS_BF_HALO_TIMEOUT) */
} htfs_peer;

/* First half of a rebuild: destination of every local particle (d_bounds: per decomposed axis HTFS_BRICK_MAX_P + 1 boundaries in
 * the positions' dtype, axis-major), stable sort by destination, migrants packed into d_mig_send (rows of 8 scalars: position,
 * velocity; row 0 of each message = its count), shifted by shift[m]. */
HTF_API int htfs_brick_migrate_pack(const htfs_brick *g, const void *d_pos, const void *d_vel, int dtype, const void *d_bounds,
                                    const htfs_brick_work *w, void *d_mig_send, unsigned *d_counts, htf_stream stream);
/* Second half, after d_mig_recv holds the neighbors' messages: candidates = [stayed | from offset index n_msg-1 | ... | from 0],
 * classed in this brick, stable sort by class, written into the two segments with inert rows behind them (position NaN, velocity 0,
 * mass kept; d_n_neigh[row] = 0 if given); counts, class boundaries, halo message sizes and overflow flags into d_counts. */
HTF_API int htfs_brick_migrate_merge(const htfs_brick *g, void *d_pos, void *d_vel, int dtype, const void *d_bounds,
                                     const htfs_brick_work *w, const void *d_mig_recv, unsigned *d_n_neigh, unsigned *d_counts,
                                     htf_stream stream);
/* Per step: the halo messages packed from the boundary segment (inert rows behind each message's count) into d_send
 * [sum_m ghost_cap[m]] Scalar4; d_ghost_direct (nullable; replica mode without a transport): also written straight into the ghost
 * region, message m at the rows its receiver -- this rank -- expects it (source offset -o). */
HTF_API int htfs_brick_pack_halo(const htfs_brick *g, const void *d_pos, int dtype, const unsigned *d_counts, void *d_send,
                                 void *d_ghost_direct, htf_stream stream);
/* the same two packers with the rows stored into the neighbors' inboxes and signalled (transport "peer"), and the receiving side */
HTF_API int htfs_brick_pack_halo_peer(const htfs_brick *g, const void *d_pos, int dtype, const unsigned *d_counts, const htfs_peer *peer,
                                      htf_stream stream);
HTF_API int htfs_brick_unpack_halo(const htfs_brick *g, void *d_pos, int dtype, const htfs_peer *peer, unsigned *d_counts,
                                   htf_stream stream);
/* htfs_nve_step over the local rows AND htfs_brick_pack_halo in one launch: every boundary row writes its new position into the
 * messages that carry it (their inert tails stay as the last rebuild's pack left them).  Same bits as the two calls. */
HTF_API int htfs_brick_nve_halo(const htfs_brick *g, void *d_pos, void *d_vel, const void *d_force, int dtype, double dt,
                                const htf_box *box, const unsigned *d_counts, void *d_send, void *d_ghost_direct, htf_stream stream);
HTF_API int htfs_brick_nve_halo_peer(const htfs_brick *g, void *d_pos, void *d_vel, const void *d_force, int dtype, double dt,
                                     const htf_box *box, const unsigned *d_counts, const htfs_peer *peer, htf_stream stream);

/* ---- the integrator (and a brick's halo pack) as the EPILOGUE of the one-kernel step (round 6).  The lanes that hold a finished
 * row's force go on with htfs_nve_step's update of that row -- v += f dt in place, x(t + dt) into d_pos_next, the OTHER position
 * buffer (every wave still reads x(t) of everybody; the caller swaps the two arrays behind the launch) -- and, for a boundary row of
 * a brick, with its new position in every halo message that carries it (htfs_brick_nve_halo's rows, found through d_row_slots).
 * A plain step is then ONE launch where it was force kernel + integrator (+ pack): same bits (tests/test_gpu_standin.py).
 * A context holds up to HTFS_EPILOGUE_SLOTS descriptors in device memory (the two directions of a ping-pong between two position
 * arrays): htfs_set_step_epilogue registers one (a blocking upload: set-up time, not the step loop), htfs_use_step_epilogue names
 * the one every later htf_compute_forces[_rows] of the context carries (-1: none) -- a host-side word, free per step.  The launch
 * honours it on the one-kernel route without a virial (htf_config.fused != 0, a built-in closed form, batch_size 0, period 1, no
 * check_nlist, fp32 positions and forces: the fp64 wire measured slower with it); *applies says whether this context will -- when not, the caller integrates as
 * before. */
#define HTFS_EPILOGUE_SLOTS 2
typedef struct htfs_step_epilogue {
    void *d_vel;                 /* Scalar4[N] */
    void *d_pos_next;            /* Scalar4[N + ghosts] */
    int dtype;                   /* HTF_F32 / HTF_F64: the Scalar of both (and of the context) */
    double dt;
    htf_box box;                 /* the integrator's box (htfs_nve_step's) */
    const htfs_brick *brick;     /* NULL: no halo pack */
    const unsigned *d_row_slots; /* [cap_bnd][HTFS_BRICK_MAX_MSG]: htfs_brick_row_slots */
    void *d_halo_send;           /* [sum ghost_cap] Scalar4 (a transport sends it), or NULL */
    void *d_ghost_direct;        /* the ghost region of d_pos_next (this rank is its own neighbor), or NULL */
    /* the MAIL of a launch (both NULL: none): two status words an earlier launch on the stream left on the device -- a
     * device-decided list's [largest row, rebuilds] -- that one lane of the force launch carries to pinned host memory (8-byte
     * aligned; one 8-byte store behind a system-scope fence: never torn) while the rows are evaluated, where a copy behind the
     * rebuild chain was a stream operation of its own.  A slot registered with mail holds a second descriptor that carries it;
     * htfs_use_step_epilogue's `mail` selects that one, for the force launch of a check step */
    const unsigned *d_mail_src;
    unsigned *h_mail_dst;
} htfs_step_epilogue;
HTF_API int htfs_set_step_epilogue(htf_ctx *ctx, int slot, const htfs_step_epilogue *ep, int *applies);
/* slot -1: none.  mail != 0: the slot's descriptor with the mail (an error when the slot was registered without) */
HTF_API int htfs_use_step_epilogue(htf_ctx *ctx, int slot, int mail);
/* d_row_slots[j][m] <- the slot of boundary row j in halo message m, 0xFFFFFFFF where the row is not in it (or beyond the message's
 * count): the class boundaries and slot table of the last re-plan, once per re-plan instead of once per row and step. */
HTF_API int htfs_brick_row_slots(const htfs_brick *g, const unsigned *d_counts, unsigned *d_row_slots, htf_stream stream);

/* ---- messages between ranks without a communication library (csrc/mailbox.hip): the migration messages of a re-plan and the
 * all-reduced distance check of transport "peer", so that every graph of a decomposed run is library-free.  Memory a neighbor's
 * kernels store into is allocated here -- fine-grained (hipExtMallocWithFlags(hipDeviceMallocFinegrained): coherent between
 * agents while kernels run, what a mapping across xGMI wants) or ordinary -- zeroed, and travels as a hipIpc handle. */
#define HTFS_IPC_HANDLE_BYTES 64
#define HTFS_MBOX_MAX_MSG 8
#define HTFS_MBOX_MAX_RANKS 64
HTF_API int htfs_shared_alloc(size_t bytes, int finegrained, void **out);
HTF_API int htfs_shared_free(void *p);
HTF_API int htfs_ipc_export(const void *p, void *handle64);          /* HTFS_IPC_HANDLE_BYTES bytes */
HTF_API int htfs_ipc_import(const void *handle64, void **out);        /* maps another process's allocation on the current device */
HTF_API int htfs_ipc_close(void *p);
/* One rank's view of a message channel.  Units are 16 bytes.  Every rank owns a mailbox of [2][half_units] units (two halves, by
 * the exchange number's parity) and one signal word per incoming message; message m of an exchange is stored at box_off[m] of the
 * receiver's half and its number published to remote_signal[m].  All ranks perform the same sequence of exchanges. */
typedef struct htfs_mailbox {
    void *remote[HTFS_MBOX_MAX_MSG];             /* message m's destination: the receiver's mailbox base */
    unsigned *remote_signal[HTFS_MBOX_MAX_MSG];  /* ... and the receiver's signal word for it */
    void *mine;                                  /* this rank's mailbox, */
    unsigned *my_signal;                         /* its signal words [n_msg], */
    unsigned *state;                             /* and [4]: exchanges done, workgroups finished, timeouts seen, spare */
    unsigned spin_limit;
    unsigned half_units;
} htfs_mailbox;
/* message m = units [send_off[m], + units[m]) of d_send -> box_off[m] of its receiver's mailbox.  row_units > 0: a message is rows
 * of that many units whose row 0 starts with its row count -- only row 0 and that many rows travel. */
HTF_API int htfs_mailbox_push(const htfs_mailbox *mb, int n_msg, const void *d_send, const unsigned *send_off, const unsigned *units,
                              const unsigned *box_off, int row_units, htf_stream stream);
/* the receiving half: message j of THIS exchange (its units at box_off[j] of my mailbox) -> units [recv_off[j], ...) of d_recv, behind
 * a bounded wait for its number; a message that does not arrive is delivered EMPTY (row count 0) and *d_flags |= flag_bit. */
HTF_API int htfs_mailbox_pull(const htfs_mailbox *mb, int n_msg, void *d_recv, const unsigned *recv_off, const unsigned *units,
                              const unsigned *box_off, int row_units, unsigned *d_flags, unsigned flag_bit, htf_stream stream);
/* d_value[0] <- max over the ranks (non-negative floats), one launch: every rank stores {exchange number, value} as one 8-byte
 * word into slot `rank` of every rank's table ([world][2] words) and polls its own.  A rank that does not answer within the spin
 * limit: the result is 3e38 (the caller rebuilds rather than trusts its list) and *d_flags |= flag_bit. */
typedef struct htfs_reduce_box {
    void *remote[HTFS_MBOX_MAX_RANKS];   /* rank r's table, r = 0 .. world - 1 (this rank's own included) */
    void *mine;
    unsigned *state;                     /* [4] */
    unsigned spin_limit;
    int world, rank;
} htfs_reduce_box;
HTF_API int htfs_mailbox_allreduce_max_f32(const htfs_reduce_box *rb, float *d_value, unsigned *d_flags, unsigned flag_bit, htf_stream stream);

#ifdef __cplusplus
}
#endif
/* the check step without a check launch (htfs_nve_step_check, htfs_rebuild_nlist_gated): part of this interface, in a file of its own */
#include "htf_step_check.h"
#endif
