/* Internal host-side data model of libcholamd (not installed; the public ABI is include/cholamd.h).
 *
 * Storage layout (the MI355X-first replacement of the mapper's per-block instances,
 * cholesky.cc:65-73): ONE contiguous fp64 arena holding one column-major PANEL per separator s.
 * Panel(s) has the separator's own columns (n_s of them) and the rows of s followed by the rows
 * of every ancestor of s in increasing permuted position (parent, grand-parent, ..., root), so
 * block (anc, s) of the reference is a row slice of panel(s) with the panel's leading dimension.
 * ROW COMPACTION: the slice of the separator itself and of its parent hold every row; the slice of a
 * higher ancestor holds only the 16-row tiles (rows 16 t .. 16 t + 15 of the ancestor) that a filled tile
 * of the block touches at the time the separator is eliminated -- the others stay zero in the reference's
 * dense block and are never read or written (blas.rg:385-395), here they have no storage
 * (chol_block.tmap / chol_block_row; lapl_3375: 13.9 -> 8.9 MB, gen 60^3: 15.2 -> 5.1 GB).
 * Panels are laid out by ascending label, hence the panels of the top
 * of the tree (root last) form a contiguous tail of the arena -- the extend-add exchange buffer of
 * the multi-GPU driver.
 */
#ifndef CHOL_PLAN_H
#define CHOL_PLAN_H

#include <stdint.h>
#include "cholamd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHOL_ENTRY_OUT 0     /* chol_plan.e_cls */
#define CHOL_ENTRY_IN 1
#define CHOL_ENTRY_DROPPED 2
#define CHOL_NB 16        /* diagonal-block width of the POTRF/TRSM kernels = one fp64 MFMA tile */
#define CHOL_RR_MAXN 272  /* largest pivot the register-resident kernels take (17 tiles) */
#ifndef CHOL_FOLLOW_ALL_MAXT
#define CHOL_FOLLOW_ALL_MAXT 4
#endif
// /* followers of at most this many column tiles take every column of their sources themselves */
#define CHOL_FOLLOW_TAIL 3     /* default of option follow_tail */
#define CHOL_FOLLOW_MAXT 10 /* most column tiles of a pivot block that follows its sources inside the program launch (chol_kernels.hip, follow_external) */
#define CHOL32_TRSM_GROUP 16 /* strips per workgroup of the fp32 throughput TRSM (k32_trsm_wt): the fp32 schedule pads every pivot block's strips to it */
#define CHOL32_MAXN 128   /* widest pivot block of the fp32 path: its lower triangle is factored out of LDS (chol_kernels_f32.hip) */

typedef struct {
  int n_int;    /* number of intervals */
  int *len;     /* boundary-list length per interval */
  int **raw;    /* boundary lists as in the file (interval t>0 indexes interval t-1) */
  int **start;  /* resolved to dof offsets inside the separator: start[t][i], i < len[t] */
} chol_clusters;

typedef struct {
  int r, c;                       /* labels */
  int lo_x, lo_y, hi_x, hi_y;     /* permuted coords, inclusive */
  int rows, cols, ld;
  int64_t off;                    /* arena offset (doubles) of the block's first stored row in column lo_y */
  int *tmap;                      /* row compaction: tmap[t] = position of the block's 16-row tile t among the tiles the panel stores, -1 = not
                                   * stored (structurally zero); NULL: every row is stored (diagonal and parent blocks, CHOLAMD_COMPACT=0) */
  int crows;                      /* rows the panel stores for this block */
} chol_block;
/* arena offset of row `row` (relative to the block) in the block's first column; rows of one filled tile, or of adjacent filled tiles, are
 * consecutive.  -1: the row has no storage */
static inline int64_t chol_block_row(const chol_block *B, int row)
{
  if (!B->tmap) return B->off + row;
  const int t = B->tmap[row / CHOL_NB];
  return t < 0 ? -1 : B->off + (int64_t)t * CHOL_NB + row % CHOL_NB;
}

/* device-side work descriptors (shared with the kernels; plain ints / int64 offsets in doubles
 * relative to a base pointer passed at launch) */
typedef struct {
  int64_t a_off;      /* diagonal block */
  int64_t dinv_off;   /* workspace offset of this separator's inverted diagonal NBxNB blocks */
  int n, lda;
  int sep;            /* label (for info reporting) */
  int col0;           /* first column of this diagonal block inside its pivot (blocked big pivots) */
  int ctr;            /* program launch: the block's progress counter (columns published) */
  int tab;            /* > 0: byte offset, from this descriptor's own address, of the block's role table (chol_potrf_table: which
                       * tile lives in which wave's register slot, the per-step work masks) -- built with the schedule instead of by every workgroup's
                       * prologue; 0: the kernel builds it */
  unsigned char sky[24]; /* tile-level skyline of the block (leaf pivots; all zero otherwise): tile (i, j) of the block is structurally zero for
                          * j < sky[i] -- its trailing updates are skipped (chol_kernels.hip, potrf_rr_body) */
} chol_potrf_desc;

/* ---- the POTRF role's deal of tiles to waves and its per-step work masks (potrf_rr_body in chol_kernels.hip), shared by the kernel and
 * by the host, which builds them with the schedule (chol_potrf_table) */
#define CHOL_RR_MAXT 17   /* tile columns of the widest register-resident pivot block */
#define CHOL_RR_NW 11     /* tile waves */
#define CHOL_RR_NHEAVY 9  /* tile waves that do not share a SIMD with the factor wave */
#define CHOL_RR_SLOTS 12  /* most tiles a tile wave owns */
#ifndef CHOL_RR_HEAVY_ONLY
#define CHOL_RR_HEAVY_ONLY 36 /* pivot blocks with at most this many register tiles (T <= 10) leave the factor wave's SIMD to the factor wave */
#endif
#define CHOL_RR_M_SOLVE0 12 /* step mask: bit s < 12 = slot s; bits 12, 13 = the wave's first / second panel tile of the step is not structurally zero */
#define CHOL_RR_M_SOLVE1 13
#define CHOL_RR_KM_ZERO 0x80 /* km: the tile is left of the block's skyline (zero in A: the prologue does not load it); the low bits: first step with a non-zero update */
#define CHOL_RR_TAB_MASK 0                                              /* int [CHOL_RR_MAXT][CHOL_RR_NW] */
#define CHOL_RR_TAB_IJ (CHOL_RR_MAXT * CHOL_RR_NW * 4)                   /* unsigned short [CHOL_RR_SLOTS][CHOL_RR_NW]: i | j << 8, 0xffff = empty */
#define CHOL_RR_TAB_KM (CHOL_RR_TAB_IJ + CHOL_RR_SLOTS * CHOL_RR_NW * 2) /* unsigned char [CHOL_RR_SLOTS][CHOL_RR_NW] */
#define CHOL_RR_TAB_BYTES ((CHOL_RR_TAB_KM + CHOL_RR_SLOTS * CHOL_RR_NW + 15) / 16 * 16)
#ifdef __HIPCC__
#define CHOL_HD __host__ __device__ __forceinline__
#else
#define CHOL_HD static inline
#endif
/* tile index -> (i, j) of the column-major enumeration of the lower triangle of a T x T tile grid */
CHOL_HD void chol_rr_tile_of_index(int idx, int T, int *ti, int *tj)
{
  int j = 0;
  while (j < T && idx >= T - j) { idx -= T - j; ++j; }
  if (j >= T) { *ti = -1; *tj = 1 << 20; } else { *ti = j + idx; *tj = j; }
}
/* Owner of tile `idx` of the reverse column-major enumeration of the tiles of columns >= 2.  Hardware waves 0, 4, 8 share a SIMD and fp64 MFMA
 * shares the DP units with the factor wave's scalar chain, so the two tile waves on that SIMD (tile-wave indices 3 and 7, "light") get 3 tiles
 * for every 5 of the nine others: tiles are dealt in rounds of 11, 9, 11, 9, 11 (= 51 per cycle; 153 tiles = 3 cycles -> 15 per heavy wave, 9
 * per light wave).  Slots grow with idx for every wave, so a wave's active tiles (column > k) are a suffix of its slots. */
CHOL_HD void chol_rr_owner(int idx, int ntl2, int *w, int *slot)
{
  if (ntl2 <= CHOL_RR_HEAVY_ONLY) { const int off = idx % CHOL_RR_NHEAVY; *w = off + off / 3; *slot = idx / CHOL_RR_NHEAVY; return; }
  const int cyc = idx / 51, pos = idx % 51;
  const int round = pos < 11 ? 0 : pos < 20 ? 1 : pos < 31 ? 2 : pos < 40 ? 3 : 4;
  const int off = pos - (round == 0 ? 0 : round == 1 ? 11 : round == 2 ? 20 : round == 3 ? 31 : 40);
  if (off < CHOL_RR_NHEAVY) { /* heavy waves in order: tile-wave indices 0,1,2,4,5,6,8,9,10 */
    *w = off + off / 3;
    *slot = cyc * 5 + round;
  } else {
    *w = off == CHOL_RR_NHEAVY ? 3 : 7;
    *slot = cyc * 3 + round / 2;
  }
}
/* the role table of an n-column block with tile skyline sky[24] (CHOL_RR_TAB_BYTES bytes; chol_schedule.c) */
void chol_potrf_table(int n, const unsigned char *sky, unsigned char *out);

typedef struct {
  int64_t l_off;      /* pivot block (n x n, ld ldl) */
  int64_t dinv_off;
  int64_t b_off;      /* first row of this row chunk inside the panel */
  int n, ldl, m, ldb; /* m rows (<= CHOL_TRSM_ROWS) */
  int flag;           /* fused POTRF+TRSM launch: index of the pivot block's POTRF descriptor in the same launch; program launch: its progress counter */
  int chan;           /* program launch: first counter of the follow channel the strip reports its column tiles on, or -1 */
  int band, pad;      /* program launch, banded leaf pivot wider than CHOL_FUSE_MAXN factored as ONE block: tile (J2, J) of its L is zero for
                       * J2 - J > band (<= 4): the strip keeps one L tile per step and wave (0: dense pivot block) */
} chol_trsm_desc;

#define CHOL_TRSM_W_MAXN 64 /* widest pivot block the one-wave-per-strip TRSM kernel takes (4 tiles); measured against k_trsm_rr: 6.6 vs 8.0 us at 32, 8.4 vs 9.6 at 64, 12.6 vs 11.1 at 128 */
#define CHOL_TRSM_WT_MAXN 144 /* widest pivot block of the throughput TRSM kernel (k_trsm_wt: one wave per strip, 12 strips per workgroup sharing the block's LDS image) */
#define CHOL_TRSM_WT_GROUP 12
#define CHOL_TRSM_WT_MIN 2048 /* strips (estimated from the panel heights) from which a step of the level schedule solves them with k_trsm_wt after a POTRF launch of its own */
#define CHOL_FUSE_MAXN 192 /* widest pivot block of a fused POTRF+TRSM launch (12 column tiles: three per wave of a strip) */
#define CHOL_FUSE_UPDATE_MAX 0 /* most 16x16 update tasks a fused launch carries (chol_schedule.c); measured on lapl_3375: 0/64/256 within noise (227 us), 900 -> 239, all -> 248: the role exists, a launch of its own is as fast */
#define CHOL_TRSM_ROWS 16

typedef struct {
  int64_t a_off, b_off; /* row 0 of the task's output sub-tile in the A rows / B rows of the source */
  int lda, ldb, k;
  int range;            /* 0: the source covers the whole sub-tile; else r0 | r1 << 8 | c0 << 16 | c1 << 24: it covers rows
                         * [r0, r1) x columns [c0, c1) of it only (grid-cell tasks: a 16x16 cell of the target block cuts
                         * through the cluster tiles of the reference) */
  int stage, pad;       /* program launch, extend-add jobs: the source may be read once the first `stage` staged waits of the job hold (0: no
                         * staged wait); a task's sources are sorted by stage */
} chol_upd_src;

typedef struct {
  int64_t c_off;      /* top-left element of this 16x16 (or smaller) output sub-tile */
  int ldc;
  short mv, nv;       /* valid rows / cols (<= 16) */
  int lower;          /* 1: diagonal sub-tile of a SYRK target, store only row >= col */
  int src_begin, src_end;
  int ar, br;         /* row offset of this sub-tile inside the A tile rows / B tile rows */
  int blk;            /* target block index (program launch: tasks of one block form the update jobs) */
} chol_upd_task;

/* ---- program launch (chol_build_program, k_program): the whole factorisation as ONE launch of resident workgroups that
 * draw jobs from a queue in a topological order and hand data to each other through counters in global memory.
 * Counters are monotonic across factorisations: a wait for `value` on counter c means  ctr[c] - epoch * total[c] >= value,
 * total[c] = what one factorisation adds to c. */
typedef struct { int ctr, value; } chol_wait;
enum chol_job_kind { CHOL_JOB_POTRF = 0, CHOL_JOB_TRSM = 1, CHOL_JOB_UPDATE = 2 }; /* chol_job.kind (a plain int: Python and the tests read the numbers) */
typedef struct {
  int kind;            /* chol_job_kind: POTRF of one pivot block, TRSM group (<= 3 strips of one pivot block), update group (16x16 tasks of one target block) */
  int first, n;        /* POTRF: descriptor index; TRSM: strips [first, first + n); update: tasks [first, first + n) */
  int wait_first, n_wait; /* chol_wait entries that must hold before the job touches its data */
  int sig[2], sig_add; /* counters raised by sig_add once the job's stores have completed (-1: none); POTRF jobs publish
                        * their column progress themselves */
  int ext_first, n_ext;/* POTRF: the external panels it follows (chol_ext), none = plain POTRF */
  int mode, n_pre;     /* n_pre: the leading waits that gate the whole job; the others are STAGED (update jobs of the extend-add: one per source
                        * pivot block in expected order of completion, chol_upd_src.stage) and are looked at by the tasks.  mode: update: 0 = one wave per task (light tasks, twelve at a time), 1 = four waves per task splitting K / the sources
                        * (heavy tasks, three at a time); POTRF job that follows and has waits: the followed item in front of whose round its own tiles
                        * are added, n_ext = after the last item (chosen by the schedule, option follow_own; a start of a round or n_ext) */
} chol_job;
typedef struct {       /* one followed column tile: (rows of the follower's block) x (16 columns of a source pivot block).  A follower's items are
                        * queued in the order their columns are EXPECTED to arrive (position of the column in its source's pivot chain: the
                        * columns of two children that run side by side alternate) -- a fixed order: the sums are the same in every run */
  int64_t off;         /* first of the follower's rows in the first column of the tile */
  int ld, ncol;        /* leading dimension of the source panel, columns of the tile (<= 16) */
  int ctr, need;       /* counter raised by every one of the `need` strips covering the rows once it has stored this column tile */
} chol_ext;
/* How a follower consumes its list of followed column tiles (follow_external): in ROUNDS of one or two items.  The grouping is a pure
 * function of (position in the list, length of the list, column tiles of the follower) -- every wave of the workgroup walks the list for
 * itself and must count the same barriers (a grouping that depended on what had been published at the time dead-locked once: the waves
 * disagreed).  Shared by the kernel and the host-side check (cholamd_follow_rounds, tests/test_host.py). */
#define CHOL_FOLLOW_PAIR_MAXT 17   /* two column tiles share an LDS buffer of this many tiles */
#define CHOL_FOLLOW_SINGLE_TAIL 0  /* last items of a list that go one by one (0 / 1 / 2 measured: 189.5 / 190.4 / 190.2 us on lapl_3375) */
#define CHOL_FOLLOW_OWN_BEFORE 2   /* the follower's own tiles go in at the last round that starts at or before item n - CHOL_FOLLOW_OWN_BEFORE (the default
                                    * place, chol_follow_own_at; the place in force is chol_job.mode, see option follow_own) */
#define CHOL_FOLLOW_OWN 1          /* default of option follow_own */
#if defined(__HIPCC__)
#define CHOL_HD __host__ __device__ __forceinline__
#else
#define CHOL_HD static inline
#endif
CHOL_HD int chol_follow_round(int i, int n_ext, int T)
{ /* items of the round that starts at item i */
  const int pair_lim = 2 * T <= CHOL_FOLLOW_PAIR_MAXT ? n_ext - CHOL_FOLLOW_SINGLE_TAIL : 0; /* items [i, i + 1] form a round while i + 1 < pair_lim */
  return i + 1 < pair_lim ? 2 : 1;
}
CHOL_HD int chol_follow_own_at(int n_ext, int T)
{ /* first item of the round in front of which the follower's own tiles are added */
  int own_at = 0;
  for (int i = 0; i < n_ext; i += chol_follow_round(i, n_ext, T))
    if (i <= n_ext - CHOL_FOLLOW_OWN_BEFORE) own_at = i;
  return own_at;
}

typedef struct {
  int n_job; chol_job *job;
  int n_wait; chol_wait *wait;
  int n_ext; chol_ext *ext;
  int n_ctr; int *ctr_total;
  int follow;          /* followers in use */
} chol_program;

/* one batched launch: descriptors [first, first + n) of the level's array of that kind */
enum chol_phase_kind { /* chol_phase.kind (a plain int: Python and the tests read the numbers) */
  CHOL_PH_POTRF = 0, CHOL_PH_TRSM = 1,
  CHOL_PH_UPDATE = 2,    /* 16x16 tasks */
  CHOL_PH_UPDATE_MT = 3, /* 64x64 macro-tile tasks */
  CHOL_PH_TRSM_W = 4,    /* every strip's pivot block <= CHOL_TRSM_W_MAXN wide */
  CHOL_PH_FUSED = 5,     /* potrf (first, n) + trsm (first2, n2) + 16x16 update tasks (first3, n3) */
  CHOL_PH_BCAST = 6,     /* distributed top levels, see chol_bcast */
  CHOL_PH_TRSM_WT = 7    /* throughput form, k_trsm_wt */
};
typedef struct {
  int kind;  /* chol_phase_kind */
  int first, n, first2, n2, first3, n3;
} chol_phase;
/* CHOL_PH_BCAST (distributed top levels): broadcast of the column blocks [first, first + n) of the level's bcast list: every rank receives
 * `count` doubles at arena offset `off` from rank `owner` */
typedef struct { int64_t off, count; int owner, heap; } chol_bcast; /* heap: heap index of the top separator the block belongs to */
/* ranks whose copy of a column block of top separator `heap` (tree level < log2(world)) can be non-zero before the extend-add exchange: the ranks
 * whose subtrees hang under the separator -- their updates are the only ones that reach it (A's entries of the block start on its owner:
 * cholamd_device_fill, which receives nothing from itself).  Bit r = rank r. */
static inline unsigned chol_top_contributors(int heap, int world)
{
  int d = 0, l = 0;
  while ((1 << d) < world) d++;
  while ((heap >> (l + 1)) > 0) l++;
  const int lo = (heap << (d - l)) - (1 << d), hi = ((heap + 1) << (d - l)) - (1 << d);
  unsigned m = 0u;
  for (int g = lo; g < hi; g++) m |= 1u << g;
  return m;
}

/* schedule switches of one device object (chol_schedule.c): read from the environment once, at cholamd_device_create */
#define CHOL_DIST_MIN 1024      /* dist_top = 2 (auto): the top levels are distributed when the root separator has this many columns */
#define CHOL_MT_MIN_TILES 8192 /* a phase whose 16x16 sub-tile count reaches this goes to 64x64 macro tiles for its larger targets */
typedef struct {
  int split_min, split_nb;  /* pivots wider than split_min are factored in column blocks of at most split_nb columns */
  int fuse;                 /* POTRF + TRSM of a column-block step in one launch */
  int fuse_update_max;      /* most 16x16 update tasks such a launch carries */
  int mt_min_tiles;
  int trsm_group;           /* unfused schedule: every pivot block's strips padded to this many, TRSM phases of kind 7 (the fp32 schedule: CHOL32_TRSM_GROUP); 0: off */
  int trsm_wt_min;          /* level schedule: steps with at least this many TRSM strips take the throughput TRSM (0: never) */
  int cells;                /* extend-add of small phases by 16x16 grid cells of the target blocks */
  int program;              /* small problems: the whole factorisation as one launch (chol_build_program) */
  int follow;               /* ... in which pivot blocks follow their children's / predecessor's TRSM strips */
  int dist_top;             /* 0 / 1 / 2 = auto (CHOL_DIST_MIN); world > 1: the levels above the cut are distributed over the ranks by column blocks (owner factors and
                             * solves a block, broadcasts it, every rank updates the column blocks it owns) instead of replicated */
  int skyline;              /* program launch: the tile-level skyline of the leaf pivots is used (zero early parts, zero tile updates skipped,
                             * banded leaves up to CHOL_RR_MAXN columns factored as one block) */
  int stage_chunk;          /* program launch: a banded leaf factored as one block hands its columns to the extend-add jobs in chunks of this many
                             * column tiles (every strip of the block then publishes its column tiles); 0: the whole block at once */
  int fine_upd;             /* program launch: followed strips wait for the update jobs into THEIR rows' block, not for all into the panel */
  int staged;               /* program launch: the extend-add jobs take their sources as the source pivots finish (staged waits) */
  int follow_tail_split;    /* the same tail for the next column block of a split pivot (one source: the strips of its own rows) */
  int follow_tail;          /* a follower wider than CHOL_FOLLOW_ALL_MAXT column tiles takes only the LAST follow_tail column tiles of each source
                             * itself; the columns before them reach its diagonal block through update jobs on other CUs (0: follows everything) */
  int merge_targets;        /* level schedule: extend-add targets (and the row runs of a panel) that are neighbours in storage are merged, so that the
                             * 64x64 macro tiles and the 16-row strips fill up (bit-identical sums) */
  int leaf_envelope;        /* level schedule: a LEAF's factor stays inside the envelope of A (nothing reaches a leaf from below), so its TRSM strips, trailing
                             * updates and extend-add sources leave out what is structurally zero: rows beyond the band of a column block, ancestor rows
                             * in front of their first entry, the columns of a source in front of its rows' first entries (identical results) */
  int super_blocks;         /* column blocks per super-block of a wide pivot: the trailing matrix beyond a super-block gets one update of
                             * rank super_blocks * (block width) instead of one per block */
  int follow_own;           /* program launch: where a follower with waits adds its own tiles (chol_job.mode).  0: in front of the round
                             * chol_follow_own_at names, everywhere; 1: after the last followed item where early update jobs write the follower's
                             * diagonal block (they end after the last early column tile is on the channel, a few column steps before the last
                             * followed one: the wait for them is over late, and in front of the last round it would hold that round up), at
                             * chol_follow_own_at everywhere else; 2: after the last item for every follower with waits.  Fixed by the plan,
                             * never by what has been published: the waves count barriers by it, and it is a position in the sum */
} chol_sched_opts;
#define CHOL_SUPER_BLOCKS 3
#define CHOL_STAGE_CHUNK 0
void chol_sched_opts_default(chol_sched_opts *o);
void chol_sched_opts_from_env(chol_sched_opts *o);

#define CHOL_SPLIT_MIN 144 /* pivots wider than this are factored in column blocks (chol_schedule.c); measured on lapl_3375: 258 us unsplit, 240 us at 144/144 */
#ifndef CHOL_PROG_SPLIT_MIN
#define CHOL_PROG_SPLIT_MIN 176
#endif
/* CHOL_PROG_SPLIT_MIN: the program launch factors pivots up to this width whole when split_min is at its default (lapl_3375: its 161 / 163 / 174-column leaves
                                * as one 11-tile block, 177.9 -> 176.4 us; the level-by-level schedule is better off at 144: 215 against 220 us) */
#define CHOL_SPLIT_NB 144  /* ... of at most this many columns */

typedef struct {
  int level;
  int n_phase; chol_phase *phase;          /* launches of this level, in order */
  int n_potrf; chol_potrf_desc *potrf;
  int n_trsm; chol_trsm_desc *trsm;
  int n_task; chol_upd_task *task;         /* 16x16 sub-tile tasks (k_update) */
  int n_task_mt; chol_upd_task *task_mt;   /* 64x64 macro-tile tasks (k_update_mt): targets larger than 16x16 */
  int n_src; chol_upd_src *src;            /* task.src_begin/src_end index this array */
  int n_bcast; chol_bcast *bcast;          /* distributed top levels: the column blocks exchanged after each step */
} chol_level_work;

/* solve-phase descriptors */
typedef struct {
  int64_t a_off; int n, lda; int x_off; int sep;
  int64_t dinv_off; /* the separator's 16x16 diagonal-block inverses in the solve workspace */
  int band;         /* > 0: L(i, j) = 0 inside the separator's diagonal block for i - j > band (a LEAF's factor stays inside the envelope of A: the solve does not
                     * read the rows of a span's panel beyond it); 0: dense */
} chol_trsv_desc;
typedef struct {
  int64_t a_off; int m, n, lda; int x_off, y_off; /* y(m) -= A x(n)  or  y(n) -= A^T x(m); one descriptor per stored row run of a block.  Forward sources of the
                                                   * target-centric level solve (chol_solve_level.fw): y_off = the run's first row inside the target separator */
  int c_lo;                                       /* the run's rows are zero in the columns [0, c_lo) (rows of a LEAF's panel start at their first entry of A); 0: unknown */
} chol_gemv_desc;

struct cholamd_plan {
  int n, nz_file, levels, nsep, max_int_size;
  char banner[160];
  MM_typecode typecode;
  int *perm;        /* dof at permuted position */
  int *iperm;       /* permuted position of dof */
  int *sep_of_pos;  /* label per permuted position */
  int *sep_size, *sep_off;        /* index 1..nsep */
  int *tree;                      /* heap index 1..nsep -> label */
  int *heap_of, *level_of;        /* label -> heap index / tree level */
  chol_clusters *cl;              /* index 1..nsep */
  int nblk; chol_block *blk;
  int *blk_index;                 /* (nsep+1)^2 -> index into blk or -1 */
  int64_t *panel_off; int *panel_ld, *panel_rows; /* per label (panel_rows: rows stored) */
  int compact;                    /* row compaction of the ancestor blocks in force */
  int64_t arena_dense;            /* what the arena would be with every ancestor row stored */
  int64_t arena;                  /* doubles */
  int64_t ws_doubles;             /* workspace (inverted diagonal blocks) */
  int64_t *dinv_off;              /* per label */
  /* tril(A) mapped into the arena */
  int64_t nnz_a, dropped; int64_t *a_dst; double *a_val;
  /* A, both triangles, CSR over ORIGINAL dof indices (residual of the iterative refinement) */
  int64_t *csr_ptr; int *csr_col; double *csr_val;
  /* the VALUE ARRAY: nz_file doubles in the order plan creation received the entries (cholamd_device_set_values).  e_row / e_col: the entry
   * list itself (original 0-based coordinates); a_src[e] / csr_src[k]: index in the value array of scatter entry e / CSR entry k (both
   * triangles point at the same index); e_cls[k]: what became of entry k -- outside the pattern (0.0 at creation: in neither list), in the
   * scatter list and the CSR, or dropped by the ordering (CSR only) */
  int *e_row, *e_col, *a_src, *csr_src; unsigned char *e_cls;
  /* in-pattern entries that share their arena position with the entry before them in the sorted scatter list (the scatter overwrites, the CSR sums: the
   * values-gradient calls refuse such a plan), and the value-array index of the first one (-1: none) */
  int64_t duplicates; int dup_first;
  /* fill snapshots per interval label */
  int64_t *snap_n; cholamd_filled **snap;
  /* reference-order BLAS call list */
  int64_t nops, cap_ops; cholamd_op *ops;
  int64_t calls[16][4]; double flops[16][4];
  int64_t nnz_l;      /* exact scalar-symbolic nnz(L) of P A P^T */
  int64_t nnz_tiles;  /* area of the filled tiles the schedule touches (>= nnz_l) */
  double fmin;        /* sum_j colcount_j^2, the lower bound F_min of SURVEY 8d */
};
typedef struct cholamd_plan plan_t; /* the host files' short name (chol_symbolic.c, chol_schedule.c, chol_lists.c) */
#define BIDX(p, r, c) ((p)->blk_index[(size_t)(r) * ((p)->nsep + 1) + (c)])

/* chol_symbolic.c */
/* the plan rules of the values-gradient calls (include/cholamd.h at cholamd_values_grad_pairs): count == nz, no dropped and no duplicate entries; 0 or
 * CHOLAMD_ERR_ARG with the message set */
int chol_values_grad_plan_ok(const struct cholamd_plan *p, int64_t count, const char *what);
int chol_plan_finish(struct cholamd_plan *p, int nz, const int *a_row, const int *a_col, const double *a_val);
const chol_block *chol_plan_block(const struct cholamd_plan *p, int r, int c);
int chol_ntiles(const struct cholamd_plan *p, int sep, int interval);
/* Build the device work lists of one tree level for (rank, world); caller frees with chol_level_work_free */
/* the whole factorisation as one program (single GPU); descriptors in `w`, jobs in `prog`; CHOLAMD_ERR_ARG (with the reason in
 * cholamd_last_error) if the problem does not qualify (a pivot block wider than CHOL_FUSE_MAXN, macro-tile phases) */
int chol_build_program(const struct cholamd_plan *p, const chol_sched_opts *opts, chol_level_work *w, chol_program *prog);
void chol_program_free(chol_program *prog);
/* host-side self-check: every wait is satisfiable by the signals of jobs the queue order lets run (simulated with `workers`
 * resident workgroups), counters total up, the jobs cover the work of the per-level lists */
int chol_program_check(const struct cholamd_plan *p, const chol_sched_opts *opts, int workers);
int chol_program_check_built(const struct cholamd_plan *p, const chol_sched_opts *opts, int workers, const chol_level_work *w, const chol_program *g);
int chol_build_level_work(const struct cholamd_plan *p, const chol_sched_opts *opts /* NULL: defaults */, int level, int rank, int world, chol_level_work *out);
void chol_level_work_free(chol_level_work *w);
int chol_owner_of(const struct cholamd_plan *p, int label, int world); /* -1: shared top of the tree */
int chol_split_level(int world);
/* the envelope of A in the LEAF panels (chol_schedule.c, at their definitions), shared with the list builders of chol_lists.c: per separator (index
 * 1..nsep, NULL unless a leaf) the first non-zero column tile of every tile row of the pivot / the first non-zero column of every panel row */
unsigned char **chol_leaf_skylines(const struct cholamd_plan *p);
void chol_free_skylines(unsigned char **sky, int ns);
int **chol_leaf_row_first(const struct cholamd_plan *p);
/* solve lists of one tree level (this and the list builders below: chol_lists.c); caller frees with chol_solve_level_free */
typedef struct {
  int n_trsv; chol_trsv_desc *trsv;                 /* one per separator of the level (forward and backward) */
  int n_fw; chol_gemv_desc *fw;                     /* forward sources, grouped by target row chunk */
  int n_grp; int *grp_start; int *grp_rows;         /* grp_start[n_grp+1]; grp_rows = (row0, y_off) pairs */
  int n_bw; chol_gemv_desc *bw; int *bw_start;      /* backward sources per separator: bw_start[n_trsv+1] */
  /* driver-level solve (cholamd_solve): the (ancestor, separator) blocks `bw` cut into row chunks, one workgroup each:
   * forward: (block index, first row, first column, first non-zero column of these rows) quadruples, chunks of CHOL_SOLVE_FW_ROWS rows x CHOL_SOLVE_COLS columns (the tall blocks of the top
   * levels are few: without the column cut 40 workgroups carried a level); backward: (first run, end run, first column, 0) quadruples -- 64 columns of
   * one separator over a range of its row runs `bw` (runs are cut at CHOL_SOLVE_BW_ROWS rows; the range is all of the separator's runs unless the level
   * then has fewer than CHOL_SOLVE_BW_ITEMS workgroups) */
  int n_ifw; int *ifw;
  int n_ibw; int *ibw;
  int max_n;                                        /* widest separator of the level */
  int max_rows_under_span;                          /* most rows any separator of the level has to read under a 256-column span (band / dense) */
  int banded;                                       /* every separator of the level is at most one span wide or a leaf with a band of at most one span: its whole
                                                     * triangle can be solved by one workgroup in one launch (k_solve_leaf32) */
} chol_solve_level;
#define CHOL_SOLVE_FW_ROWS 256
#define CHOL_SOLVE_BW_ROWS 1024
#define CHOL_SOLVE_BW_COLS 64
#define CHOL_SOLVE_BW_ITEMS 4096
#define CHOL_SOLVE_COLS 1024
int chol_build_solve_level(const struct cholamd_plan *p, int level, chol_solve_level *out);
int chol_build_solve_level_part(const struct cholamd_plan *p, int level, int rank, int world, chol_solve_level *out);
void chol_solve_level_free(chol_solve_level *w);
/* the TRSV descriptors of all levels (count of them, sorted in place by x_off) as the diagonal walk of cholamd_factor_diag / _logdet: prefix[count + 1] =
 * columns before each descriptor; an error unless they tile the permuted vector exactly once inside the arena */
int chol_diag_list(const struct cholamd_plan *p, chol_trsv_desc *list, int count, int *prefix);

/* ---- selected inversion (cholamd_selinv; chol_selinv.hip): the lists of one tree level.  The unit of the recursion is a COLUMN BLOCK of at most
 * CHOL_SELINV_W columns of a separator, last block first; its "rows below" are the rows panel(s) stores after the block's last column (the separator's
 * own rows, then the stored rows of the ancestors).  A panel's rows are cut into TILES of at most 16 rows on the 16-row grid of the separator they belong
 * to (the grid of chol_block.tmap), in storage order = ascending permuted position.  chain = the separator and its ancestors, bottom up (chain index 0 =
 * the separator itself).  rowoff[tile][k] = arena offset, in column 0 of panel(chain[k]), of the tile's first row -- chol_block_row of block
 * (tile's separator, chain[k]) -- or -1: chain[k] lies above the tile's separator (only the lower triangle is stored) or the row compaction of that panel
 * dropped the tile.  Z(i, j), i in tile a, j in tile b, a after b (or a == b and i >= j), lives at
 *   rowoff[a][tile[b].k] + (i - tile[a].pos0) + (j - chain_pos0[tile[b].k]) * chain_ld[tile[b].k]        (Z arena = the arena's own layout)
 * and reads as 0.0 where rowoff is -1. */
#define CHOL_SELINV_W 64
#define CHOL_SELINV_MAX_TILES 65535 /* most 16-row tiles of a panel (they lie on grid.y of the step launches): a panel of 10^6 stored rows; build_selinv refuses more */
typedef struct { int q0, nrows, pos0, k; } chol_selinv_tile; /* first row inside the panel, rows (<= 16), permuted position of the first row, chain index of its separator */
typedef struct {
  int64_t panel_off;           /* arena offset of panel(s) */
  int64_t ws_off;              /* workspace of the separator: Y^T (prows x W, row-major), Z[below, J]^T (the same shape), L_JJ^-1 (W x W, column-major) */
  int64_t rowoff_first;        /* rowoff[rowoff_first + tile * nchain + k] */
  int ld, w, prows, nblk;      /* leading dimension, columns, stored rows, column blocks */
  int sep;
  int tile_first, ntile, nown; /* tiles [tile_first, tile_first + ntile) of the level's list; the first nown are the separator's own rows */
  int chain_first, nchain;     /* chain_ld / chain_pos0 [chain_first + k] */
  int pad;
} chol_selinv_sep;
typedef struct {
  int level;
  int n_sep; chol_selinv_sep *sep;     /* ordered by column blocks, most first: the separators that take part in step t (block nblk - 1 - t) are a prefix */
  int n_tile; chol_selinv_tile *tile;
  int n_chain; int *chain_ld, *chain_pos0;
  int64_t n_rowoff; int64_t *rowoff;
  int max_nblk, max_tiles;
  int64_t ws_doubles;
} chol_selinv_level;
int chol_build_selinv_level(const struct cholamd_plan *p, int level, chol_selinv_level *out);
void chol_selinv_level_free(chol_selinv_level *w);

/* ---- Schur complement on the top k levels of the tree (cholamd_schur; chol_schur.hip).  The kept separators (heap indices 1 .. 2^k - 1) are the tail
 * [t0, n) of the permuted order; Schur coordinate i = permuted position t0 + i.  A PIECE is one 16-row tile of a block (r, c) of two kept separators, r at or
 * after c in the permuted order, over the block's columns (a diagonal block: the columns up to the tile's last row -- the lower triangle), optionally cut
 * into chunks of `chunk` columns.  off = arena offset of the piece's first element, or -1: the block does not exist (r, c not ancestor and descendant) or
 * the row compaction dropped the tile -- structurally zero; with_empty = 0 leaves those out (the host view cholamd_plan_schur_list), with_empty = 1 makes the
 * pieces tile the lower triangle of S exactly once (the gather kernel's list: it writes the zeros too).  diag: only row0 + i >= col0 + j is meant. */
#define CHOL_SCHUR_CHUNK 64 /* columns of a piece of the gather kernel's list: one workgroup moves 16 x 64 */
typedef struct { int64_t off; int ld, rows, cols, row0, col0, diag; } chol_schur_desc;
int chol_schur_range(const struct cholamd_plan *p, int k, int *t0_out); /* m (the kept dofs), *t0_out = n - m; < 0: error */
int64_t chol_schur_pieces(const struct cholamd_plan *p, int k, int with_empty, int chunk /* 0: whole */, int64_t cap, chol_schur_desc *out); /* the count, whatever cap */
void chol_set_error(const char *fmt, ...);

/* ---- forward product with the factor (cholamd_multiply_half; chol_multiply.hip): ONE list for the whole tree and each direction.  An ITEM owns
 * nv <= CHOL_MUL_TILE consecutive positions y[y_off ..] of the permuted result -- a 16-row chunk of a separator on its 16-row grid (FORWARD, y = L z) or a
 * 16-column chunk of a separator (BACKWARD, y = L^T z) -- and sums over its SOURCES [src_first, src_end) in list order; no other item writes them.
 * A source is a strip of stored entries, the item's 16 lines wide and `len` reduction steps long, z[z_off + k] being the factor of step k:
 *   FORWARD   line i = a row,    L(i, k) = arena[a_off + i + k * ld],  meant iff k <= tri + i  (diagonal block: the lower triangle; else tri is large)
 *   BACKWARD  line j = a column, L(k, j) = arena[a_off + k + j * ld],  meant iff k >= tri + j  (diagonal block: tri = 0; else tri = -CHOL_MUL_TILE)
 * FORWARD sources: the separator's own diagonal block rows (from the first column the leaf band allows), then the chunk's rows in the panel of every
 * descendant that stores them (row compaction: chol_block_row), level by level downwards, from the first column c_lo the leaf envelope allows.
 * BACKWARD sources: the diagonal block's rows from the chunk's first column (down to what the leaf band allows), then the stored row runs of the panel,
 * parent first (the runs of the solve's `bw` list, uncut), a leaf's run left out where the chunk lies in front of its c_lo. */
#define CHOL_MUL_TILE 16
typedef struct { int64_t a_off; int ld, len, z_off, tri; } chol_mul_src;
typedef struct { int src_first, src_end, y_off, nv; } chol_mul_item;
typedef struct {
  int n_item[2]; chol_mul_item *item[2]; /* [CHOLAMD_HALF_FORWARD], [CHOLAMD_HALF_BACKWARD] */
  int n_src[2]; chol_mul_src *src[2];
} chol_mul_lists;
int chol_build_multiply(const struct cholamd_plan *p, chol_mul_lists *out);
void chol_mul_lists_free(chol_mul_lists *w);

/* ---- deterministic streamed solve (option solve_deterministic; chol_solve_det.hip): the sweeps of cholamd_solve with every off-diagonal contribution GATHERED by
 * the owner of its target instead of scattered with atomics.  A STEP is one gather launch over its items [item_first, item_end), y[item] -= sum over the
 * item's sources in list order, followed -- where col0 >= 0 -- by the diagonal solve of the 256-column span [col0, col0 + CHOL_SDET_SPAN) of every
 * separator of the step's tree level wider than col0 (the span solvers of the streamed solve, plain stores).  Every level has one LEAD step (col0 = -1: no
 * span) for what reaches it from outside its own diagonal blocks, then one step per span for what reaches the span from inside the block.  FORWARD runs the
 * levels leaves first and span 0 first, BACKWARD root first and the last span first.  Items and sources are those of chol_mul_lists (one workgroup per
 * item, 16 lines):
 *   FORWARD   lead: a 16-row chunk's rows in the panel of every descendant that stores them (the FORWARD multiply sources without the diagonal block);
 *             span: a 16-row chunk's rows in the separator's own diagonal block over the columns [first column the leaf band allows, col0)
 *   BACKWARD  lead: the stored row runs of a 16-column chunk's columns into the ancestors (the BACKWARD multiply sources without the diagonal block);
 *             span: the rows [col0 + CHOL_SDET_SPAN, end the leaf band allows) of a 16-column chunk's columns in the own diagonal block
 * Every source of a step was solved by an earlier step and no item of the step owns it; a chunk without sources has no item.  Within a step every permuted
 * position has at most one owner, and over a sweep every position is solved exactly once (chol_build_solve_det checks both).  Ordering between steps comes
 * from kernel boundaries on the stream alone.  The lead step runs the long descendant lists of ALL chunks of a wide separator side by side; attached to
 * the spans they would run sixteen at a time, one span after the other. */
#define CHOL_SDET_SPAN 256
typedef struct { int level, col0, item_first, item_end; } chol_sdet_step;
typedef struct {
  int n_step[2]; chol_sdet_step *step[2]; /* [CHOLAMD_HALF_FORWARD], [CHOLAMD_HALF_BACKWARD] */
  int n_item[2]; chol_mul_item *item[2];
  int n_src[2]; chol_mul_src *src[2];
} chol_sdet_lists;
int chol_build_solve_det(const struct cholamd_plan *p, chol_sdet_lists *out);
void chol_sdet_lists_free(chol_sdet_lists *w);
/* The same lists CUT at level k for the Schur condense / expand (device option schur_deterministic; include/cholamd.h at cholamd_schur_condense_nrhs): FORWARD
 * the steps of the levels levels - 1 .. k and one KEPT LEAD step (level = -1, col0 = -1: the lead-step sources of the kept chunks that read positions under
 * the cut), BACKWARD the steps of the levels k .. levels - 1.  Checks its own invariants as chol_build_solve_det does. */
int chol_build_schur_det(const struct cholamd_plan *p, int k, chol_sdet_lists *out);
/* The same lists PRUNED to a set of separators per direction for the sparse solve (cholamd_sparse_*; chol_lists_sparse.c).  act_fw / act_bw
 * are indexed by separator label (1 .. nsep) and closed under "parent" (chol_sparse_masks closes them).  Derived from the full lists, in their order:
 *   FORWARD   an item stays iff the separator of its y_off is in act_fw, a source of it iff the separator of its z_off is (a dropped source multiplies
 *             positions that are exactly zero); an item left without sources goes
 *   BACKWARD  an item stays iff its separator is in act_bw; its sources lie in ancestors, hence in act_bw (checked)
 *   a span step (col0 >= 0) stays iff an active separator of its level is wider than col0, with or without items; a lead step stays iff it has items -- or had
 *   none in the full lists either and its level holds an active separator (it launches nothing; with both masks all ones the output is the full lists)
 * trsv[q]: the chol_trsv_desc of the active separators (q = 0, 1: of the direction; 2: of the union, the 16x16 inverses of a whole solve), level by level in
 * the order of chol_solve_level.trsv: level l = [lvl_first[q][l], lvl_first[q][l + 1]), the widest of them lvl_max_n[q][l] columns.  range: the positions of
 * the union's separators as n_range ascending (pos0, len) pairs, neighbours merged; n_pos of them in all.  Checks its own invariants (CHOLAMD_ERR_INVARIANT):
 * over a sweep every active position is solved exactly once, no source reads a position that is inactive for its direction or not solved yet, no item owns
 * an inactive position, every source strip lies inside the arena. */
typedef struct {
  chol_sdet_lists w;
  int n_act[3]; chol_trsv_desc *trsv[3]; int *lvl_first[3], *lvl_max_n[3];
  int n_range; int *range; int64_t n_pos;
} chol_sparse_lists;
int chol_build_sparse_det(const struct cholamd_plan *p, const unsigned char *act_fw, const unsigned char *act_bw, chol_sparse_lists *out);
void chol_sparse_lists_free(chol_sparse_lists *w);
void chol_sparse_counts(const struct cholamd_plan *p, const chol_sparse_lists *w, int64_t out[12]); /* the layout of cholamd_plan_sparse_counts */
/* the masks of a pair of dof lists (original order): act_fw = up(in), act_bw = up(out), nsep + 1 bytes each; pos_in / pos_out (may be NULL): the dofs'
 * permuted positions.  CHOLAMD_ERR_ARG with the first offender named: a NULL, a count < 1, a dof outside [0, n), a duplicate inside either list */
int chol_sparse_masks(const struct cholamd_plan *p, const char *what, const int *in_dofs, int n_in, const int *out_dofs, int n_out, unsigned char *act_fw, unsigned char *act_bw,
                      int *pos_in, int *pos_out);
/* the two halves of a step of the block host walk (chol_lists.c at sdet_host_block_sweep): the gather of the step's items with the kernel's partition, and
 * the substitution inside the span [col0, col0 + CHOL_SDET_SPAN) of ONE separator; yp = the permuted row-major block (n x 32) */
void chol_sdet_host_block_gather(const chol_sdet_lists *w, int which, const chol_sdet_step *st, const double *arena, double *yp);
void chol_sdet_host_block_span(const struct cholamd_plan *p, int sep, int col0, int which, const double *arena, double *yp);

/* ---- block form of the products (cholamd_multiply_half_nrhs; chol_multiply_nrhs.hip): the same items and sources on a chunk of 32 columns.  The reduction
 * range of a source is cut into CHUNKS of CHOL_MULN_KSTEP steps; chunk c of the s-th source of an item (s counted from the item's first) belongs to wave
 * chol_muln_wave(s, c) of the item's CHOL_MULN_WAVES waves -- round robin, turned by the source's number so that an item of many short sources (one chunk
 * each) spreads over all waves too.  A wave adds its chunks in list order into its own 16 x 32 partial tile, the CHOL_MULN_WAVES tiles are added in wave
 * order.  chol_muln_elem is the operand of line `line` and step `k` of a source: the arena index, CLAMPED into the strip (line < nv, k < len: a tile is read
 * whole, its reads stay inside the strip), and *meant = whether the entry takes part -- it is a line the item owns, a step the source has, and on or below
 * the diagonal of a diagonal block (the `tri` rule of chol_mul_src).  An operand that is not meant is SELECTED to 0.0, never multiplied by zero.  The
 * kernel and cholamd_plan_multiply_host_nrhs both use these two functions, so the host walk checks the kernel's index logic.  So do the block gather of the
 * deterministic solve (k_solve_det_gather_nrhs, option solve_deterministic_block) and its host walk cholamd_plan_solve_det_host_nrhs, on the items and
 * sources of chol_sdet_lists.
 * Precondition of chol_muln_elem: nv >= 1 and q->len >= 1 (the clamp is to nv - 1 and len - 1).  chol_build_multiply makes no other item or source -- an
 * item has 1 .. 16 positions, a source of no steps is not pushed -- and a chunk loop over [0, len) does not run for len = 0. */
#define CHOL_MULN_KSTEP 32 /* reduction steps of one chunk: 8 MFMA steps of 4 whose loads are in flight together */
#define CHOL_MULN_WAVES 4
CHOL_HD int chol_muln_wave(int s, int c) { return (s + c) & (CHOL_MULN_WAVES - 1); }
CHOL_HD int64_t chol_muln_elem(const chol_mul_src *q, int backward, int nv, int line, int k, int *meant)
{
  const int lc = line < nv ? line : nv - 1, kc = k < q->len ? k : q->len - 1;
  *meant = line < nv && k < q->len && (backward ? k >= q->tri + line : k <= q->tri + line);
  return q->a_off + (backward ? (int64_t)kc + (int64_t)lc * q->ld : (int64_t)lc + (int64_t)kc * q->ld);
}

/* ---- low-rank corrections on the finished factor (cholamd_lowrank_*; chol_lowrank.hip, chol_lowrank_host.c): the partition of the three tall-skinny
 * kernels, shared by the kernels and their host restatements.
 *   T = P^T Q (n rows summed away): the rows are cut into SLABS of CHOL_LR_SLAB rows, slab s = rows [s CHOL_LR_SLAB, min(n, (s + 1) CHOL_LR_SLAB)) -- a
 *     function of n alone, never of k, m or the grid.  One workgroup per slab walks it in blocks of CHOL_LR_STAGE rows (staged in LDS, four rows per MFMA
 *     step) and keeps the slab's partial 16 x 16 tiles in registers: tile number `id` of a call belongs to wave id % CHOL_LR_WAVES, slot id / CHOL_LR_WAVES.
 *     The tiles of the Gram form (P == Q) are the lower ones in row-major order of the triangle (chol_lr_gram_tile), those of the general form (m <= 32
 *     columns per call) tile id = (id / mt, id % mt).  A second launch adds the partials of an element in slab order.
 *   X = alpha X + beta V T: one workgroup per chunk of CHOL_LR_ROWS rows; wave w takes the 32-column chunks w, w + 4, ... of X.  A call of at most 32 columns
 *     (the corrected solves) shares its one chunk instead: the k / 4 reduction steps are cut into CHOL_LR_RWAVES consecutive ranges
 *     of ceil(steps / CHOL_LR_RWAVES), one per wave, and the waves' partial tiles are added in wave order.
 *   w_i = sum_j W_ij^2: one thread per row, j ascending. */
#define CHOL_LR_MAX 256      /* most columns of U (CHOLAMD_LOWRANK_MAX) */
#define CHOL_LR_SLAB 1024    /* rows of a slab of the transposed product */
#define CHOL_LR_STAGE 32     /* rows staged in LDS at a time (8 MFMA steps) */
#define CHOL_LR_WAVES 16     /* waves of a slab's workgroup */
#define CHOL_LR_SLOTS 9      /* tiles a wave can own: ceil(136 / 16), 136 = lower tiles of a 256 x 256 Gram matrix */
#define CHOL_LR_ROWS 16      /* rows of a chunk of the row-owned product */
#define CHOL_LR_RWAVES 4     /* waves of its workgroup */
CHOL_HD int64_t chol_lr_slabs(int64_t n) { return (n + CHOL_LR_SLAB - 1) / CHOL_LR_SLAB; }
CHOL_HD int chol_lr_gram_tiles(int kt) { return kt * (kt + 1) / 2; }
CHOL_HD void chol_lr_gram_tile(int id, int *ti, int *tj)
{ /* id = ti (ti + 1) / 2 + tj, tj <= ti */
  int r = 0;
  while ((r + 1) * (r + 2) / 2 <= id) r++;
  *ti = r; *tj = id - r * (r + 1) / 2;
}

#ifdef __cplusplus
}
#endif
#endif
