/*
 * cholamd.h -- C ABI of the MI355X-native supernodal Cholesky hot path.
 *
 * This is the drop-in boundary for ONE path of syamajala/cholesky: the per-supernode
 * POTRF / TRSM / SYRK / GEMM frontal updates driven by the nested-dissection separator tree
 * (reference: mmat.rg:1227-1355 -> blas.rg:292-504 -> libcblas/liblapacke).  Plain pointers and
 * sizes only; no torch / HIP types appear in any signature (streams are passed as void*).
 *
 * Three nested levels are exported, each replacing a reference interface (file:line cited at each
 * declaration, paths relative to the reference tree):
 *
 *   L-A  BLAS level   -- what Terra links today (blas.rg:18-22, mmat.rg:29-30): the six CBLAS /
 *                        LAPACKE entry points with the exact parameter combinations the reference
 *                        uses.  Host pointers in, host pointers out (like the CPU library they
 *                        replace); `_dev` variants take device pointers + stream.
 *   L-B  task level   -- the four `fused_*` leaf tasks (blas.rg:292-504): one call = one task =
 *                        one batched HIP launch over the task's list of filled tiles.
 *   L-C  driver level -- what `main` does around them (mmat.rg:1097-1362): ingest, symbolic
 *                        analysis, A scatter, the level schedule, factor/solution writers, solve.
 *
 * All functions return 0 on success unless stated otherwise.  Errors are never silent: there is no
 * CPU fallback anywhere in this library -- if no HIP device is usable, every compute entry point
 * returns CHOLAMD_ERR_NO_DEVICE.
 */
#ifndef CHOLAMD_H
#define CHOLAMD_H

#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ----------------------------------------------------------------------------------------- */
/* error codes                                                                                 */
/* ----------------------------------------------------------------------------------------- */
#define CHOLAMD_OK 0
#define CHOLAMD_ERR_IO (-1)          /* fopen/parse failure (the reference leaves these unchecked, mnd.c:33,84,161,209) */
#define CHOLAMD_ERR_FORMAT (-2)      /* file violates the on-disk contract */
#define CHOLAMD_ERR_INVARIANT (-3)   /* ordering/cluster invariant the reference relies on is violated */
#define CHOLAMD_ERR_ARG (-4)         /* unsupported parameter combination */
#define CHOLAMD_ERR_NO_DEVICE (-5)   /* no usable HIP device: there is NO CPU fallback */
#define CHOLAMD_ERR_HIP (-6)         /* a HIP runtime call failed (see cholamd_last_error) */
#define CHOLAMD_ERR_NOMEM (-7)
#define CHOLAMD_ERR_COMM (-9)        /* an RCCL call failed (see cholamd_last_error) */
#define CHOLAMD_ERR_STALL (-8)       /* cholamd_factor_info only: a workgroup of a fused launch gave up waiting (~50 ms) for a progress
                                      * word of the same launch; the factor in the arena is NOT valid */
/* > 0: LAPACK-style info of the first failing pivot (see cholamd_factor_info) */

const char *cholamd_last_error(void);
const char *cholamd_version(void);

/* ----------------------------------------------------------------------------------------- */
/* Matrix-Market ingest: the four mmio.c entry points the reference calls                       */
/*   mm_read_banner        mmio.c:96-179   (called mmat.rg:81)                                  */
/*   mm_read_mtx_crd_size  mmio.c:189-217  (called mmat.rg:91)                                  */
/*   mm_write_banner       mmio.c:406-415  (called mmat.rg:128)                                 */
/*   mm_write_mtx_crd_size mmio.c:181-187  (called mmat.rg:129)                                 */
/* Same names, same argument meaning, same return codes (mmio.h:73-79), so libmmio.so's users    */
/* can link this library instead.  Like the reference, mm_read_banner does NOT run mm_is_valid,  */
/* so the fixtures' "real hermitian" banner is accepted.  One deliberate difference:             */
/* mm_write_mtx_crd_size returns 0 when the size line was written; the reference compares        */
/* fprintf's character count with 3 (mmio.c:181-187) and so reports MM_COULD_NOT_WRITE_FILE for   */
/* every successful write -- a return value its only caller ignores (mmat.rg:129).                */
/* ----------------------------------------------------------------------------------------- */
typedef char MM_typecode[4];
#define MM_COULD_NOT_READ_FILE 11
#define MM_PREMATURE_EOF 12
#define MM_NOT_MTX 13
#define MM_NO_HEADER 14
#define MM_UNSUPPORTED_TYPE 15
#define MM_LINE_TOO_LONG 16
#define MM_COULD_NOT_WRITE_FILE 17

int mm_read_banner(FILE *f, MM_typecode *matcode);
int mm_read_mtx_crd_size(FILE *f, int *M, int *N, int *nz);
int mm_write_banner(FILE *f, MM_typecode matcode);
int mm_write_mtx_crd_size(FILE *f, int M, int N, int nz);
char *mm_typecode_to_str(MM_typecode matcode); /* mmio.c:488-511; caller frees */

/* ----------------------------------------------------------------------------------------- */
/* Separator / cluster / matrix / vector readers: plain-array equivalents of mnd.h:28-66        */
/* (the reference versions write into Legion accessors; the file formats are the contract).     */
/* ----------------------------------------------------------------------------------------- */
typedef struct cholamd_sepinfo { int levels; int num_separators; } cholamd_sepinfo; /* SepInfo, mnd.h:23-26 */

/* read_separators (mnd.c:22-69).  idx_out[pos] = original dof at permuted position pos,
 * sep_out[pos] = 1-based separator label; both of length dim. */
int cholamd_read_separators(const char *file, int dim, int *idx_out, int *sep_out, cholamd_sepinfo *info);

/* read_clusters (mnd.c:71-150).  Emits the flat (idx, interval, sep) triples in file order, at
 * most cap of them; *count_out = number available.  Returns max_int_size (>= 0) like the
 * reference, or a negative error code. */
int cholamd_read_clusters(const char *file, int *idx_out, int *interval_out, int *sep_out, int64_t cap, int64_t *count_out);

/* read_matrix (mnd.c:152-199): nz coordinate entries, 0-based, as stored in the file (the
 * reference hashes them; here they come back as plain COO arrays). */
int cholamd_read_matrix(const char *file, int nz, int *row_out, int *col_out, double *val_out);

/* read_vector (mnd.c:201-229): skips three header lines blindly, then n values. */
int cholamd_read_vector(const char *file, int n, double *out);

/* ----------------------------------------------------------------------------------------- */
/* L-C: plan (host) = ingest + symbolic analysis of mmat.rg:1097-1209, re-expressed as plain C  */
/* ----------------------------------------------------------------------------------------- */
typedef struct cholamd_plan cholamd_plan;

/* Filled tile descriptor: fspace Filled, blas.rg:55-61 (filled == 0 means FILLED, sic). */
typedef struct cholamd_filled {
  int filled;
  int sep_x, sep_y;       /* block colour: (row separator, col separator), 1-based labels */
  int interval;           /* interval label of the snapshot */
  int cluster;            /* tile id z = row * ncols + col */
  int lo_x, lo_y, hi_x, hi_y; /* rect2d bounds, inclusive, permuted matrix coordinates */
} cholamd_filled;

/* One reference BLAS call of the level schedule, in the reference's program order. */
typedef struct cholamd_op {
  int op;                 /* 0 POTRF, 1 TRSM, 2 SYRK, 3 GEMM */
  int level;
  int m, n, k;
  int a_sx, a_sy, a_z;    /* A tile colour */
  int b_sx, b_sy, b_z;    /* B tile colour (0 if unused) */
  int c_sx, c_sy, c_z;    /* C tile colour (0 if unused) */
} cholamd_op;

int cholamd_plan_create(const char *matrix_file, const char *separator_file, const char *clusters_file, cholamd_plan **out);
/* Same, from arrays already in memory (generated problems).  perm[pos] = dof; sep_sizes by label
 * 1..nsep; clusters as (idx, interval, sep) triples like cholamd_read_clusters emits; A as COO
 * lower triangle (row >= col), 0-based original coordinates. */
int cholamd_plan_create_from_arrays(int n, int levels, const int *perm, const int *sep_sizes,
                                    const int *cl_idx, const int *cl_interval, const int *cl_sep, int64_t cl_count,
                                    int64_t nz, const int *a_row, const int *a_col, const double *a_val,
                                    const char *banner, cholamd_plan **out);
void cholamd_plan_destroy(cholamd_plan *p);

int cholamd_plan_n(const cholamd_plan *p);
int cholamd_plan_nz(const cholamd_plan *p);
int cholamd_plan_levels(const cholamd_plan *p);
int cholamd_plan_num_separators(const cholamd_plan *p);
int cholamd_plan_max_int_size(const cholamd_plan *p);
int cholamd_plan_num_blocks(const cholamd_plan *p);
int64_t cholamd_plan_arena_doubles(const cholamd_plan *p);   /* size of the panel arena */
/* Row compaction.  panel(s) stores the rows of s and of its parent in full; of every higher ancestor only the 16-row tiles (rows 16 t ..
 * 16 t + 15 of the ancestor) that a filled tile of block (ancestor, s) touches when s is eliminated -- the rest of the reference's dense
 * block instance stays zero and is never touched (blas.rg:385-395).  CHOLAMD_COMPACT=0 in the environment at plan creation stores every
 * row (the round-1/2 layout).  arena_dense_doubles: the size without compaction; block_tile_map: out[t] = stored position of tile t of
 * block (r, c) in units of 16 rows from the block's first stored row, -1 = not stored; returns the number of tiles. */
int64_t cholamd_plan_arena_dense_doubles(const cholamd_plan *p);
int cholamd_plan_block_tile_map(const cholamd_plan *p, int r, int c, int *out);
int64_t cholamd_plan_dropped_entries(const cholamd_plan *p); /* entries of A outside every allocated block */
const char *cholamd_plan_banner(const cholamd_plan *p);
void cholamd_plan_perm(const cholamd_plan *p, int *out);          /* n ints */
void cholamd_plan_sep_sizes(const cholamd_plan *p, int *out);     /* nsep ints, by label */
void cholamd_plan_sep_offsets(const cholamd_plan *p, int *out);   /* nsep ints, by label */
void cholamd_plan_tree(const cholamd_plan *p, int *out);          /* nsep ints: heap index-1 -> label (mmat.rg:834-849) */
/* per allocated block, ordered by (row label, col label): r, c, lo_x, lo_y, hi_x, hi_y, ld, and
 * the block's offset (in doubles) inside the arena split into two ints (lo32, hi32): 9 ints */
void cholamd_plan_blocks(const cholamd_plan *p, int *out);
/* snapshot `interval_lbl` of compute_filled_clusters (mmat.rg:1000-1016), filled tiles only,
 * ordered by (row label, col label, cluster) */
int64_t cholamd_plan_snapshot_count(const cholamd_plan *p, int interval_lbl);
void cholamd_plan_snapshot(const cholamd_plan *p, int interval_lbl, cholamd_filled *out);
/* the reference's BLAS call list (program order of mmat.rg:1227-1355) and its work */
int64_t cholamd_plan_num_ops(const cholamd_plan *p);
void cholamd_plan_ops(const cholamd_plan *p, cholamd_op *out);
void cholamd_plan_counts(const cholamd_plan *p, int level /* -1 = all */, int64_t calls[4], double flops[4]);
double cholamd_plan_flops(const cholamd_plan *p);           /* F_ref, SURVEY 8d */
int64_t cholamd_plan_nnz_a(const cholamd_plan *p);          /* nnz(tril A) kept */
int64_t cholamd_plan_nnz_l(const cholamd_plan *p);          /* exact symbolic nnz(L) of P A P^T (scalar elimination tree) */
int64_t cholamd_plan_nnz_tiles(const cholamd_plan *p);      /* area of the filled tiles the schedule stores (>= nnz(L)) */
double cholamd_plan_fmin(const cholamd_plan *p);            /* F_min = sum_j colcount_j^2 */
int64_t cholamd_plan_alg_bytes(const cholamd_plan *p);      /* B_alg = 8 (nnz(tril A) + nnz(L)) */

/* fill_block for every block (mmat.rg:529-633, 1216-1224): zero the arena and scatter A. */
int cholamd_plan_fill_host(const cholamd_plan *p, double *arena);
/* ---- the VALUE ARRAY: cholamd_plan_nz() doubles in the order in which plan creation received the entries (file order for cholamd_plan_create,
 * array order for _from_arrays, the generator's own order for _from_problem); entry k of the array is the value of entry k of that list.  It is how
 * new values of A on the same pattern reach a plan's consumers (here on the host; cholamd_device_set_values on the device).  The plan itself is
 * immutable: its own values, the writers and cholamd_plan_fill_host are what they were at creation.
 * Entries that were exactly 0.0 at creation are OUTSIDE THE PATTERN: invisible to the reference (mnd.c:168-195), they have no place in the scatter
 * list or the residual operator, and no later value can give them one (that is a new plan).
 * cholamd_plan_entries: the entry list in value-array order (original 0-based coordinates, as stored: a symmetric file's entry stays on its side of
 * the diagonal), so a caller need not re-read the file to know the order.
 * cholamd_plan_value_map: src_out[e] = index in the value array of scatter entry e, cholamd_plan_nnz_a() of them in the order of the scatter
 * (ascending arena offset); the value-array indices that do not occur are out of the pattern or were dropped by the ordering
 * (cholamd_plan_dropped_entries; those stay in the residual operator).
 * cholamd_plan_fill_host_values: cholamd_plan_fill_host with the value array `vals` instead of the plan's own values; count != cholamd_plan_nz()
 * or a NULL array: CHOLAMD_ERR_ARG, nothing written. */
int cholamd_plan_entries(const cholamd_plan *p, int *row, int *col);
int cholamd_plan_value_map(const cholamd_plan *p, int64_t *src_out);
int cholamd_plan_fill_host_values(const cholamd_plan *p, const double *vals, int64_t count, double *arena);
/* where the factor's diagonal lies in an arena (the walk of cholamd_factor_diag / cholamd_factor_logdet, host side): one descriptor per separator, ordered
 * by permuted position -- element j < cols[i] of descriptor i is arena[a_off[i] + j * (lda[i] + 1)] and is L(x_off[i] + j, x_off[i] + j); prefix[i] = columns
 * before descriptor i, prefix[count] = n.  Every array has room for cholamd_plan_num_separators() entries (prefix: one more) and may be NULL.  Returns the
 * number of descriptors, or a negative error code if they do not cover every permuted position exactly once. */
int cholamd_plan_diag_list(const cholamd_plan *p, int64_t *a_off, int *cols, int *lda, int *x_off, int *sep, int *prefix);
/* Multi-GPU view of the same: with `world` ranks the shared top of the tree (the tail of
 * the arena starting at *tail_offset_out) receives A's entries on rank 0 only, so that the sum over
 * ranks of the tails after the local levels equals A_top minus every contribution. */
int cholamd_plan_fill_host_part(const cholamd_plan *p, double *arena, int rank, int world, int64_t *tail_offset_out);
/* sizes of the device work lists of one tree level for (rank, world): potrf descriptors, trsm
 * strips, update tasks, update sources */
int cholamd_plan_level_work_counts(const cholamd_plan *p, int level, int rank, int world, int out[4]);
/* the volumes of cholamd_plan_level_work_volume (single GPU) under the level schedule's merging switch (option merge_targets) and macro-tile
 * threshold (mt_min_tiles, < 0: default), plus the list lengths: out[6..8] = 16x16 tasks, 64x64 macro-tile tasks, TRSM strips */
int cholamd_plan_level_work_volume_opts(const cholamd_plan *p, int level, int merge_targets, int mt_min_tiles, int64_t out[9]);
/* how full the 64 x 64 macro-tile update tasks of a level are (single GPU): out = { tasks, tasks with all 64 x 64 elements valid,
 * sum of valid elements x depth, sum of tile elements x depth } */
int cholamd_plan_level_mt_fill(const cholamd_plan *p, int level, int64_t out[4]);
/* what the macro-tile update kernels (k_update_mt, k32_update_mt) meet on a level's lists for (rank, world), built as the device builds them
 * under options merge_targets, mt_min_tiles (< 0: default) and dist_top; f32 != 0: the fp32 schedule (pivot blocks of at most 128 columns).
 * out[] is indexed by the constants below (Plan.MT_CLASSES names them in the same order); sources are counted once per task that reads them */
enum {
  CHOLAMD_MT_TASKS,          /* macro-tile tasks */
  CHOLAMD_MT_FULL,           /* ... with mv == nv == 64 */
  CHOLAMD_MT_EDGE_DMA,       /* edge tasks the kernel serves by LDS-DMA (its bound check against the arena's length holds) */
  CHOLAMD_MT_EDGE_STAGED,    /* edge tasks it stages through registers (the check fails) */
  CHOLAMD_MT_LOWER,          /* `lower` tasks */
  CHOLAMD_MT_LOWER_AR,       /* `lower` tasks with ar != 0 */
  CHOLAMD_MT_MV1,            /* tasks with mv == 1 */
  CHOLAMD_MT_NV1,            /* tasks with nv == 1 */
  CHOLAMD_MT_MAX_SOURCES,    /* most sources of one task */
  CHOLAMD_MT_SOURCES_32,     /* tasks with exactly 32 sources */
  CHOLAMD_MT_SOURCES_33_63,  /* ... with 33 .. 63 */
  CHOLAMD_MT_SOURCES_64,     /* ... with 64 or more */
  CHOLAMD_MT_K_SHORT,        /* sources with k < 16 */
  CHOLAMD_MT_K_CHUNKS,       /* k >= 16 and k % 16 == 0 */
  CHOLAMD_MT_K_CHUNKS_1,     /* k >= 16 and k % 16 == 1 */
  CHOLAMD_MT_K_OTHER,        /* other k */
  CHOLAMD_MT_ODD_ORIGIN,     /* sources with an odd operand origin (a_off + ar or b_off + br) */
  CHOLAMD_MT_LATE_CHUNKS,    /* tasks of more than 32 sources with a source of k >= 16 behind the 32nd (the ring issues chunks in a later descriptor batch) */
  CHOLAMD_MT_LOWER_AR_CUT,   /* `lower` tasks with ar % 64 != 0 (a SYRK target cut at a column block of the distributed top) */
  CHOLAMD_MT_EMPTY_RING,     /* DMA-served tasks (full or edge) all of whose sources have k < 16 */
  CHOLAMD_MT_DMA_SLACK,      /* the least distance, over the DMA-served edge tasks, between the furthest element their DMA touches and the arena's last element (-1: none) */
  CHOLAMD_MT_CLASSES
};
int cholamd_plan_level_mt_classes(const cholamd_plan *p, int level, int merge_targets, int mt_min_tiles, int f32, int rank, int world, int dist_top,
                                  int64_t out[CHOLAMD_MT_CLASSES]);
/* volumes of the same lists with the top levels replicated (dist_top = 0) or distributed by column blocks (1; 2 = automatic):
 * POTRF columns, TRSM elements, update volume (target elements x source depth), broadcast entries, broadcast doubles, checksum
 * of the broadcast list (the same on every rank) */
int cholamd_plan_level_work_volume(const cholamd_plan *p, int level, int rank, int world, int dist_top, int64_t out[6]);
/* volume of the extend-add exchange of (rank, world) under dist_top 0 / 1 / 2 (auto), in arena elements: received, sent, the tail,
 * column-block pieces (0 pieces: the all-reduce of the replicated top levels) -- the host-side count behind cholamd_exchange_volume.
 * Path-aware since round 4: only the blocks of the top separators on the sender's own root path travel */
int cholamd_plan_exchange_volume(const cholamd_plan *p, int rank, int world, int dist_top, int64_t out[4]);
/* the column-block pieces of that exchange (the broadcast lists of the levels above the cut): out[i] = { arena offset, elements, owner rank, heap index
 * of the top separator }, at most `max` of them; returns their number (< 0: error).  A rank sends piece i to its owner iff it does not own it and
 * its subtree hangs under that separator: the reference touches a C tile only where the fill marks it (blas.rg:385-395), and the fill of a top
 * block comes from A (scattered on the block's owner by cholamd_device_fill) and from the subtrees under it */
int cholamd_plan_exchange_pieces(const cholamd_plan *p, int world, int dist_top, int max, int64_t (*out)[4]);
/* host-side self-check of the one-launch program cholamd_factor() runs for small problems on one GPU (chol_build_program):
 * simulated with `workers` resident workgroups and every counter raised only on job completion, no job may starve; counters
 * total up; pivot blocks and TRSM rows equal those of the per-level lists.  0 = consistent, otherwise cholamd_last_error()
 * says what is wrong (also when the problem does not qualify for the program launch).  follow: with / without followers. */
int cholamd_plan_program_check(const cholamd_plan *p, int follow, int workers);
/* the same with followers under other values of the options "follow_tail", "split_min", "split_nb" (negative: the default); the other
 * switches as the environment sets them at the time of the call */
int cholamd_plan_program_check_opts(const cholamd_plan *p, int follow_tail, int split_min, int split_nb, int workers);
/* ... and under other values of "follow_tail_split" and "follow_own" (the place of the followers' own tiles) */
int cholamd_plan_program_check_follow(const cholamd_plan *p, int follow_tail, int follow_tail_split, int follow_own, int split_min, int split_nb, int workers);
int cholamd_plan_program_counts(const cholamd_plan *p, int follow, int out[6]);
/* the rounds (of one or two followed column tiles) in which a following POTRF job of `tile_columns` column tiles consumes a list of n_ext items --
 * the kernel's own grouping, a function of the list alone; and the following jobs of a plan's program: (job, items, tile columns, waits) each */
int cholamd_follow_rounds(int n_ext, int tile_columns, int cap, int *rounds_out, int *own_at_out);
int64_t cholamd_plan_program_followers(const cholamd_plan *p, int64_t cap, int *out);
/* the following jobs under given options (negative: the default), five ints each: job, items, tile columns, the item in front of whose round the
 * job adds its own tiles (items: after the last one) -- the place the schedule has chosen (option "follow_own"), which the kernel takes from the job;
 * cholamd_follow_rounds names the default place -- and wait-list entries (0: the job loads its own tiles first).  Returns the number of jobs. */
int64_t cholamd_plan_program_follow_own(const cholamd_plan *p, int follow_tail, int follow_tail_split, int follow_own, int split_min, int split_nb, int64_t cap, int *out);
/* write hazards between the update jobs of the program under given options (negative: the default): out = pairs of update jobs that write a common arena
 * element, pairs among them whose later job may start before the earlier one has completed (worked out from what the counters guarantee), the first such pair */
int cholamd_plan_program_hazards(const cholamd_plan *p, int follow_tail, int follow_tail_split, int follow_own, int split_min, int split_nb, int out[4]);
int64_t cholamd_plan_program_jobs(const cholamd_plan *p, int follow, int64_t cap, int *out); /* diagnostic dump of the job queue (scripts/prog_trace.py) */ /* jobs, following POTRF jobs, update tasks, strips, counters, followed panels */
/* dense N x N col-major image of an arena (zeros outside allocated blocks) and back */
int cholamd_plan_arena_to_dense(const cholamd_plan *p, const double *arena, double *dense);
/* write_matrix (mmat.rg:102-147): banner, "M N nnz", "row col %0.8g" per non-zero, block by
 * block; full_precision != 0 writes %.17g instead (needed for the 1e-10 gate). */
int cholamd_plan_write_matrix(const cholamd_plan *p, const double *arena, const char *file, int full_precision);
/* write_solution (mmat.rg:785-798): n lines "%0.8g" (or %.17g), original dof order, no header */
int cholamd_write_solution(const char *file, const double *x, int n, int full_precision);
/* the reference's -d structured log lines: Block lines + the POTRF / TRSM / GEMM lines of the whole op list (blas.rg:308,340,405),
 * from the symbolic phase alone (no device) */
int cholamd_plan_write_debug_log(const cholamd_plan *p, FILE *f);
/* what the reference's symbolic phase prints with -d: Block (mmat.rg:331), per level Cluster (mmat.rg:396,432) and Fill
 * (mmat.rg:1010) lines; the op lines are printed by the fused tasks as they run (cholamd_factor_debug) */
int cholamd_plan_write_debug_header(const cholamd_plan *p, FILE *f);
/* write_blocks' text dump (mmat.rg:183-217): `header`, then every allocated block with its values as "%0.2f, " */
int cholamd_plan_write_blocks_txt(const cholamd_plan *p, const double *arena, const char *file, const char *header);
int cholamd_plan_ntiles_at_level(const cholamd_plan *p, int sep, int level);

/* ----------------------------------------------------------------------------------------- */
/* Problem generator (absent from the reference, whose orderings come from an      */
/* external tool): d-dimensional 5-/7-point Laplacian on an nx x ny x nz grid (nz = 1 for 2-D),   */
/* natural index x + nx*y + nx*ny*z, diagonal 2*dim, off-diagonal -1, lower triangle -- exactly    */
/* the fixtures' matrices -- with a geometric nested-dissection ordering of `levels` tree levels  */
/* (split the longest side at its middle plane) and cluster lists that satisfy the invariants of  */
/* SURVEY A.3 (tiles of about `tile` dofs at interval 0, halved per interval, ONE tile at the      */
/* interval in force when a separator is eliminated).  Outputs are in the reference's on-disk      */
/* formats (Appendix A) so that the reference, the oracle and this library read the same files.    */
/* ----------------------------------------------------------------------------------------- */
typedef struct cholamd_problem cholamd_problem;
int cholamd_generate_laplacian(int nx, int ny, int nz, int levels, int tile, cholamd_problem **out);
void cholamd_problem_destroy(cholamd_problem *g);
int cholamd_problem_n(const cholamd_problem *g);
int cholamd_problem_nz(const cholamd_problem *g);
/* writes <prefix>.mtx, <prefix>_ord_<levels>.txt, <prefix>_clust_<levels>.txt and B_<n>x1.mtx-style
 * rhs (b_i = 1 + (7919 i mod 10)) as <prefix>_B.mtx */
int cholamd_problem_write(const cholamd_problem *g, const char *prefix);
/* plan straight from memory (no files) */
int cholamd_plan_create_from_problem(const cholamd_problem *g, cholamd_plan **out);
void cholamd_problem_rhs(const cholamd_problem *g, double *b);

/* ----------------------------------------------------------------------------------------- */
/* L-C: device side.  The arena (all per-separator panels, col-major, contiguous) lives in HBM. */
/* ----------------------------------------------------------------------------------------- */
typedef struct cholamd_device cholamd_device;

int cholamd_device_count(void);
/* Uploads the level schedule (op descriptors) of `plan` to device `device_id`. */
int cholamd_device_create(const cholamd_plan *plan, int device_id, cholamd_device **out);
void cholamd_device_destroy(cholamd_device *d);
/* device memory owned by the library (hipMalloc); callers may instead pass their own buffers
 * (e.g. torch tensors) of cholamd_plan_arena_doubles() doubles to the calls below.
 * CHOLAMD_POISON=1 in the environment (a test switch, read at every allocation): every buffer of floating-point data the library
 * allocates -- these, cholamd_device_alloc_arena's (owned ranges and scratch chunk), the work and solve vectors, the per-call BLAS
 * buffers -- gets a guard tail and starts as 0xFF bytes (NaN in fp64 and fp32) instead of whatever the allocator returns.  A read of
 * memory a kernel does not own then shows up as NaN.  Integer, flag and descriptor buffers are never poisoned.  Unset or 0: plain
 * hipMalloc, nothing else changes. */
int cholamd_device_alloc(cholamd_device *d, int64_t doubles, double **dptr);
int cholamd_device_free(cholamd_device *d, double *dptr);
int cholamd_device_upload(cholamd_device *d, double *d_dst, const double *h_src, int64_t doubles, void *stream);
int cholamd_device_download(cholamd_device *d, double *h_dst, const double *d_src, int64_t doubles, void *stream);
int cholamd_device_sync(cholamd_device *d, void *stream);
/* STREAMS.  `stream` is a hipStream_t (NULL: the null stream).  Everything a call enqueues goes to that stream, and where a call "synchronises" it waits
 * for that stream alone.  "Asynchronous on `stream`" describes a WARM call: the first call of a family on a device object also builds, uploads and
 * clears that family's lists, scratch and status words with blocking copies on the null stream, and a clearing synchronises the whole device once, so
 * that it is ordered before work on any stream (a non-blocking stream does not wait for the null stream); later calls allocate nothing and only enqueue.
 * A device object serves ONE stream of work at a time: its scratch and its counters are shared by all its calls. */
/* A scatter on the device (fill_block, mmat.rg:1216-1224): zero d_arena, scatter tril(A).  A partitioned device (cholamd_device_set_partition)
 * scatters every entry under the cut and, of the shared top of the tree, the entries exactly one rank must start from: all of them on rank 0 when the
 * top levels are replicated, those of the column blocks the rank OWNS when they are distributed (option dist_top) -- fill after set_partition /
 * set_option, with the schedule the factorisation will use. */
int cholamd_device_fill(cholamd_device *d, double *d_arena, void *stream);
/* ---- new values of A on the same pattern, from DEVICE memory, without a new plan (Newton / interior-point steps, time stepping, shifted systems).
 * d_vals: a device array of count = cholamd_plan_nz() doubles, the value array described at cholamd_plan_entries.  One gather pass on `stream`
 * replaces every copy of A's values the device object holds: the scatter list of cholamd_device_fill / _fill_f32 (the column blocks a partitioned
 * device owns included, also when cholamd_device_set_option / _set_partition rebuild them later), and the operator of cholamd_residual and of every
 * refinement.  After it every entry point that takes the device object behaves as that of a device object on a plan created from the same entries
 * with these values.  Schedules, work lists, the program, the solve lists and the plan are NOT touched, arenas already filled neither: fill again,
 * then factor.  The values belong to the device object: two objects on one plan hold independent values, and every rank object of a multi-rank run
 * needs the call.  d_vals is read during the call's kernels only.  The first call on a device object uploads the index lists (and the residual
 * operator, if no refinement has done so); later calls allocate nothing.
 * Zeros: an in-pattern entry may become 0.0 -- it is stored and factored as an explicit zero.  An entry OUTSIDE the pattern (0.0 at creation) cannot
 * become non-zero: envelope, skylines and solve bands were derived from the creation-time pattern.
 * flags = 0: the call looks at the values first (one synchronisation of `stream`, 32 bytes read back); an out-of-pattern entry that is not +-0.0 makes
 * it return CHOLAMD_ERR_ARG naming the first such entry, and the device object's PREVIOUS values stay in force.
 * flags = CHOLAMD_VALUES_NOCHECK: asynchronous on `stream`, no synchronisation; such values are ignored (they have no slot anywhere).
 * count != cholamd_plan_nz(), a NULL pointer, a negative or unknown flag: CHOLAMD_ERR_ARG, nothing written.
 * NaN / inf / values outside float's range are not refused here: the fp64 path takes them as a plan created with them would (the pivot checks report
 * what they do), and the fp32 range rule (at cholamd_device_fill_f32) follows the CURRENT values: it names the value-array index of the first
 * in-pattern value that is non-zero and not a normal float in magnitude (read back lazily, once per set_values, by the first fp32 entry point).
 * cholamd_device_values_status: the counts of the most recent cholamd_device_set_values call, accepted or refused (synchronises `stream` if they have
 * not been read yet): out[0] in-pattern values that are non-zero and not a normal float in magnitude (|v| > FLT_MAX or < FLT_MIN, NaN and inf
 * included), out[1] the smallest value-array index of one (-1: none), out[2] out-of-pattern entries whose value is not +-0.0, out[3] the smallest
 * index of one (-1: none).  Before the first call: CHOLAMD_ERR_ARG. */
#define CHOLAMD_VALUES_NOCHECK 1
int cholamd_device_set_values(cholamd_device *d, const double *d_vals, int64_t count, int flags, void *stream);
int cholamd_device_values_status(cholamd_device *d, void *stream, int64_t out[4]);
/* The hot path: the whole level loop of mmat.rg:1227-1355 on d_arena, asynchronously on stream.  Small problems (every
 * pivot block <= 192 columns, no macro-tile phase: the reference's fixtures) run as ONE launch of resident workgroups that
 * draw POTRF / TRSM / update jobs from a queue and hand data to each other through counters (option "program"); otherwise,
 * per tree level and column-block step of its pivots: one fused POTRF+TRSM launch and the update launch(es).  level_lo/level_hi
 * restrict the loop to tree levels [level_lo, level_hi] (inclusive; pass 0, levels-1 for everything) -- used by
 * the multi-GPU driver to run subtree levels and top levels separately.
 * A device object carries one workspace (diagonal-block inverses, progress words of the fused launches, info):
 * it serves one factorisation or solve at a time; use one object per concurrent stream of work.  The arena is
 * the caller's: any number of arenas can be factored one after the other with the same object.
 * Co-residency of the one-launch form: its workgroups wait for each other inside the launch.  The job list is checked when the
 * device object is built (simulated with four resident workgroups, counters raised on job completion: a list that cannot make
 * progress that way is not used, the per-level launches are); on a GPU shared with other kernels a job may wait for a producer
 * that is not resident yet -- every in-launch wait gives up after about two seconds of polling and the factorisation then FAILS
 * through info = CHOLAMD_ERR_STALL (cholamd_factor_info), it never hangs.  A stalled factorisation has written part of the arena:
 * refill (cholamd_device_fill) before factoring again; option "program" = 0 selects the per-level launches, which need no
 * co-residency beyond one launch. */
int cholamd_factor(cholamd_device *d, double *d_arena, void *stream);
int cholamd_factor_levels(cholamd_device *d, double *d_arena, int level_hi, int level_lo, void *stream);
/* Restrict the schedule to the subtrees owned by `rank` of `world` (a power of two <= 2^(levels-1)):
 * separators below the split level that are not in this rank's subtrees are skipped.  world == 1
 * restores the full schedule. */
int cholamd_device_set_partition(cholamd_device *d, int rank, int world);
/* diagnostic: one program launch with per-job clock stamps.  out (cap >= 5 * jobs int64) receives per job, in queue order:
 * kind (0 POTRF, 10 POTRF that follows, 1 TRSM group, 2 update group), then the 100 MHz real-time clock (10 ns ticks since the
 * first job was drawn) when the job was drawn, when its waits were over and when it ended, and the workgroup that ran it.
 * *njobs_out = number of jobs (call with cap = 0 to size the buffer). */
int cholamd_device_program_trace(cholamd_device *d, double *d_arena, void *stream, int64_t cap, int64_t *out, int *njobs_out);
/* diagnostic: device buffers the library itself owns in this process right now (caller-owned allocations are not counted); no device access */
int64_t cholamd_debug_live_buffers(void);
/* Debug mode of the reference (mmat.rg -d <dir>): the level loop of mmat.rg:1227-1355 LITERALLY -- one fused task
 * at a time through the task-level entry points below, serialised -- printing the tasks' POTRF / TRSM / GEMM lines on stdout
 * and, after every task, dumping the whole matrix as write_blocks does (mmat.rg:174-218): <dir>/<gen_filename>.mtx
 * (write_matrix format) and .txt (block dump), with gen_filename's names (mmat.rg:149-172: potrf_lvlL_aXY,
 * trsm_lvlL_aXY_bXY, gemm_lvlL_aXY_bXY_cXY, the block colours printed with %d%d as the reference does) and its
 * "filename: ..." lines.  Slow by design; the factor it leaves in d_arena equals cholamd_factor's to rounding. */
int cholamd_factor_debug(cholamd_device *d, double *d_arena, const char *dir, int full_precision, void *stream);
/* LAPACK-style info after the stream has been synchronised: 0 ok; k > 0 = leading minor k of the
 * pivot of separator *sep_out is not positive definite (the reference ignores this, blas.rg:71);
 * < 0 = the factorisation itself failed (CHOLAMD_ERR_STALL, or a HIP error code of this call) and
 * cholamd_last_error() says why -- callers must not use the factor in either non-zero case.
 * info belongs to the device object: in a multi-rank factorisation a rank reports the pivots it factored itself (its subtrees; of the shared top all
 * of them, or under "dist_top" its own column blocks) and otherwise 0 or a later pivot that NaN reached.  A caller must read EVERY rank's info: the
 * factor is good only if all are 0, and the first failing pivot is the smallest permuted position reported (sep_offsets[*sep_out - 1] + info - 1). */
int cholamd_factor_info(cholamd_device *d, int *sep_out);
/* Schedule / kernel-selection switches of this device object.  They default to the values the environment gave when
 * the object was created (CHOLAMD_SPLIT_MIN, CHOLAMD_SPLIT_NB, CHOLAMD_NO_FUSE, CHOLAMD_FUSE_UPDATE_MAX,
 * CHOLAMD_MT_MIN_TILES, CHOLAMD_NO_CELLS, CHOLAMD_SOLVE_REFERENCE_SHAPE, CHOLAMD_SOLVE_DETERMINISTIC: read once, there); names: "split_min",
 * "split_nb", "fuse", "fuse_update_max", "mt_min_tiles", "cells", "solve_reference_shape", "solve_deterministic" (the bit-reproducible
 * streamed solve, see "deterministic solve" below; neither of the two solve options rebuilds the work lists), "schur_deterministic" (the Schur condense / expand on
 * deterministic step lists, see cholamd_schur_condense_nrhs; CHOLAMD_SCHUR_DETERMINISTIC; rebuilds nothing), "program" (the whole factorisation
 * of a small problem as one launch; CHOLAMD_NO_PROGRAM), "follow" (its pivot blocks follow their children's TRSM strips;
 * CHOLAMD_NO_FOLLOW), "follow_tail" (followers of more than four tile columns take the last follow_tail column tiles of each source
 * themselves, update jobs bring the rest; 0 = they take everything; CHOLAMD_FOLLOW_TAIL; "follow_tail_split": the same for the next
 * column block of a split pivot), "follow_own" (where a follower that waits for update jobs adds its own tiles to the followed sums: 0 = in front
 * of the round of its last two followed column tiles; 1, the default = after the last followed column tile where early update jobs write its diagonal
 * block, as 0 elsewhere; 2 = after the last one for every such follower; the factor differs between the values by rounding; CHOLAMD_FOLLOW_OWN), "staged" (the extend-add jobs of the
 * program launch take their sources pivot block by pivot block as those are solved instead of waiting for all of them;
 * CHOLAMD_NO_STAGED), "fine_upd" (followed strips wait for the update jobs into their own rows' block only; CHOLAMD_NO_FINE_UPD),
 * (the program launch factors pivots up to 176 columns whole while "split_min" / "split_nb" are at their defaults: CHOL_PROG_SPLIT_MIN),
 * "trsm_wt_min" (level schedule: a column-block step with at least this many TRSM strips launches its POTRFs on their own and solves
 * the strips with the throughput kernel, one wave per strip; 0 = never; CHOLAMD_TRSM_WT_MIN),
 * "skyline" (program launch: the tile-level skyline of the leaf pivots -- the envelope of A inside the block -- is used: tile updates and
 * panel tiles left of it are skipped, banded leaves up to 272 columns are factored as one block; CHOLAMD_NO_SKYLINE), "stage_chunk" (such a
 * leaf's columns reach the extend-add jobs in chunks of this many column tiles; 0 = the whole block at once, the default;
 * CHOLAMD_STAGE_CHUNK),
 * "leaf_envelope" (level schedule: a leaf's factor stays inside the envelope of A, so the strips, trailing updates and extend-add sources of the leaves
 * leave out what is structurally zero -- identical factors, 16-35 % less time on the generated grids; CHOLAMD_NO_LEAF_ENVELOPE),
 * "super_blocks", "dist_top" (0 / 1 / 2 = automatic: top levels of a partitioned run distributed by column
 * blocks, see Multi-GPU below; CHOLAMD_DIST_TOP).  Rebuilds the work lists. */
int cholamd_device_set_option(cholamd_device *d, const char *name, int value);
/* number of broadcast phases in the partitioned schedule (> 0: the top levels are distributed by column blocks, option "dist_top",
 * and cholamd_factor_levels over them needs a communicator: use cholamd_factor_sharded / cholamd_factor_multi) */
int cholamd_device_bcast_phases(const cholamd_device *d);
/* Solve phase, mmat.rg:1364-1495: b and x in ORIGINAL dof order (device pointers, n doubles).
 * The off-diagonal blocks accumulate into the vector with hardware fp64 atomics, so x agrees from run to run to
 * rounding (~1e-16 relative), NOT bit for bit -- unless option "solve_deterministic" is set (below: the streamed sweeps with every contribution
 * gathered by its owner, fp64 and fp32 factor), or option "solve_reference_shape", which selects the deterministic per-call
 * kernels of the BLAS-level entry points instead (fp64 factor only, slow beyond ~10^5 unknowns).
 * What the streamed solve does NOT read: the structural zeros of the leaf panels (cholamd_plan_solve_skips; CHOLAMD_SOLVE_NO_BAND=1 in the environment
 * when the device object builds its solve lists reads everything).  The levels of at most 128 separators wider than 256 columns are solved with EXPLICIT
 * inverses of their 256-column diagonal spans (formed from the factor at the start of a solve -- of a refinement: its corrections reuse them -- in
 * 512 KiB of device memory per span: 0.4 GB for a 100^3 grid; CHOLAMD_SOLVE_NO_INV256=1 keeps the substitution form).  Their span steps hand data
 * between workgroups INSIDE a launch behind flags; the waits are bounded like the program launch's, and one that gives up poisons its part of the
 * vector with NaN (a residual or refinement then reports it) instead of hanging the device. */
int cholamd_solve(cholamd_device *d, const double *d_arena, const double *d_b, double *d_x, void *stream);
/* ---- deterministic solve: device option "solve_deterministic" (cholamd_device_set_option, or CHOLAMD_SOLVE_DETERMINISTIC non-zero in the environment at
 * cholamd_device_create; default off -- with it off nothing changes, not even which kernels run).  THE CONTRACT: with the option on, cholamd_solve,
 * cholamd_solve_f32, cholamd_solve_half, cholamd_solve_half_f32 and every solve inside cholamd_solve_refine return the SAME BITS for the same arena and the
 * same right-hand side -- from call to call, from one device object of a plan to another, in place or out of place, and BACKWARD(FORWARD(b)) equals the solve
 * bit for bit.  Hence cholamd_solve_refine takes the same number of corrections and returns the same x and relres every time.
 * How: the sweeps run level by level in STEPS.  A level's lead step is one gather launch that subtracts what reaches the level from outside its own
 * diagonal blocks -- FORWARD: a 16-row chunk's rows in the panels of its descendants; BACKWARD: a 16-column chunk's stored row runs into the ancestors.
 * Then, per 256-column span of the level's separators, one gather launch subtracts what reaches the span from inside the block (FORWARD: the chunk's
 * rows left of the span; BACKWARD: its rows below the span) and one launch solves the span.  One owner per position, sources summed in a fixed
 * list order, NO floating-point atomics; the span itself is solved out of LDS by the streamed solve's span kernels with plain stores.  Steps are ordered by
 * kernel boundaries on the stream alone: no workgroup waits for another inside a launch, there are no flags.  The 16x16 inverses are formed per call (kept
 * across the corrections of a refinement); the 256-column explicit inverses and the step launches are not used.  Structural zeros of the leaves, row
 * compaction and the upper triangles (never read) are treated as by cholamd_multiply_half, whose owner lists these are derived from.  The lists are built and
 * uploaded at the first such solve on a device object (setting the option builds nothing).
 * Precedence: where "solve_reference_shape" is also set and applies (the fp64 factor), it wins.
 * The _nrhs entry points (cholamd_solve_nrhs, cholamd_solve_half_nrhs, their _f32 forms, cholamd_solve_refine_nrhs) go COLUMN BY COLUMN through the
 * deterministic single-vector solve under the option, as they do under "solve_reference_shape": column j has the bits of the single solve of column j --
 * unless option "solve_deterministic_block" is set too (next paragraph).
 * BLOCK FORM: device option "solve_deterministic_block" (cholamd_device_set_option, or CHOLAMD_SOLVE_DETERMINISTIC_BLOCK non-zero in the environment at
 * cholamd_device_create; default off; setting it rebuilds nothing).  It has an effect only where "solve_deterministic" is on, "solve_deterministic_block" is
 * on and "solve_reference_shape" is off; in every other combination every entry point does exactly what it does without it, down to which kernels run.
 * Where the three hold, cholamd_solve_nrhs, cholamd_solve_half_nrhs, their _f32 forms and every solve inside cholamd_solve_refine_nrhs walk the same step
 * lists on chunks of 32 columns: per step one block gather (16 x 32 tiles on v_mfma_f64_16x16x4_f64, four waves per item, their partial tiles added in wave
 * order by the element's owner) and one launch of the block solve's span kernel in its substitution form, plain stores.  One pass over L and one launch
 * chain per 32 columns instead of one per column; no floating-point atomic, no flag, no wait inside a launch.  EVERY chunk takes the block kernels, whatever
 * its column count (nrhs = 1 included: a caller with one column has cholamd_solve).  THE CONTRACT of the block form:
 *  (a) the same bits for the same arena and the same B -- from call to call, from one device object of a plan to another, on a device object created under
 *      CHOLAMD_POISON=1, in place (X == B, ldx == ldb) and with ldb, ldx > n;
 *  (b) COLUMN INDEPENDENCE: the bits of column j of X depend on the arena and on column j of B only -- not on nrhs, not on the column's position (its chunk,
 *      its half of the 32-column tile), not on the other columns' contents: a NaN in another column never reaches it;
 *  (c) cholamd_solve_half_nrhs(BACKWARD) of cholamd_solve_half_nrhs(FORWARD) of B equals cholamd_solve_nrhs(B) bit for bit;
 *  (d) cholamd_solve_refine_nrhs called twice returns the same iters, the same relres per column and the same bits of X.  Column independence does NOT
 *      hold for the refinement: the columns of a chunk share the number of corrections;
 *  (e) rows n .. ld - 1 of X and columns >= nrhs are never written.
 * NOT PROMISED: the bits of the single-vector deterministic solve (the sums are partitioned differently); the two agree to rounding.
 * NOT COVERED by the block form either: the sharded and multi-GPU solves, and anything under "solve_reference_shape".
 * NOT COVERED (they keep the atomic path whatever the option says): the sharded and multi-GPU solves (cholamd_solve_sharded, cholamd_solve_multi, the
 * sharded refinement) on more than one rank.  The Schur condense / expand have an option of their own, "schur_deterministic" (at cholamd_schur_condense_nrhs
 * below); the two solve options do not reach them.
 * Needs the COMPLETE factor in the arena, like cholamd_solve: a single-GPU device object, or rank 0's after a gather.
 * cholamd_plan_solve_det_host: the same walk on the HOST over a host arena with the same lists (which = CHOLAMD_HALF_FORWARD, CHOLAMD_HALF_BACKWARD, or -1:
 * the whole solve = FORWARD then BACKWARD; b and x n doubles in original dof order, x == b allowed); a span is solved by substitution inside its own lower
 * triangle.  Deterministic, but not the device's bits (the span kernels order their sums differently).  Builds the lists anew at every call.
 * cholamd_plan_solve_det_host_nrhs: the BLOCK form on the host (which as above; B, X: n x nrhs column-major in original dof order with leading dimensions
 * ldb, ldx >= n, X == B allowed with ldx == ldb; nrhs = 0 returns 0 and touches nothing; the argument rules of cholamd_plan_multiply_host_nrhs).  A gather
 * uses the block kernel's own partition (chol_muln_wave, chol_muln_elem of chol_plan.h: four partial sums per element, added in wave order), so the host
 * walk checks the kernel's index logic; a span is solved by substitution inside its own lower triangle.  Deterministic, every column independent of the
 * others (contract (b) and (c) hold on the host too), but NOT the device's bits: the device's span kernel sums in another order.
 * cholamd_plan_solve_det_counts: out = { FORWARD steps, items, sources, entries of L read, BACKWARD steps, items, sources, entries of L read }; a step is one
 * gather launch where it has items, followed by one span launch unless it is a level's lead step; the entries are those of the gather sources plus the
 * spans' own lower triangles.
 * cholamd_plan_solve_det_lists: the lists of one direction as int64 rows, sized by the counts: steps (level, first column of the span or -1: the level's
 * lead step, first item, end item),
 * items (first permuted position, positions, first source, end source), sources (arena offset, leading dimension, reduction steps, first permuted position
 * read, triangle rule of chol_mul_src). */
int cholamd_plan_solve_det_host(const cholamd_plan *p, const double *arena_host, int which, const double *b, double *x);
int cholamd_plan_solve_det_host_nrhs(const cholamd_plan *p, const double *arena_host, int which, const double *B, int64_t ldb, double *X, int64_t ldx, int nrhs);
int cholamd_plan_solve_det_counts(const cholamd_plan *p, int64_t out[8]);
int cholamd_plan_solve_det_lists(const cholamd_plan *p, int which, int64_t *steps, int64_t *items, int64_t *srcs);
/* ---- mixed precision (BASELINE config 5; not in the reference, whose arithmetic is fp64 CBLAS throughout): fp32 factor +
 * fp64 iterative refinement.  The fp32 arena has the fp64 arena's element layout: cholamd_plan_arena_doubles() FLOATS.
 * The fp32 schedule factors pivots in blocks of at most 128 columns out of LDS (v_mfma_f32 kernels, one launch per phase);
 * info as for the fp64 path (cholamd_factor_info).  cholamd_solve_f32 is one solve with the fp32 factor (vectors and
 * arithmetic fp64, L converted on load); cholamd_solve_refine iterates x += (L32 L32^T)^-1 (b - A x) with the residual
 * in fp64 against the matrix file's A until ||b - A x|| / ||b|| <= tol or max_iter corrections have been applied, and
 * returns the corrections used and the final relative residual.  cholamd_residual computes that residual for any x
 * (d_r may be NULL); both synchronise the stream.
 * fp32 range: every non-zero entry of A must be a normal float in magnitude (FLT_MIN <= |a| <= FLT_MAX); otherwise cholamd_device_fill_f32, the fp32
 * factorisations (cholamd_factor_f32, _levels_f32, _sharded_f32, _multi_f32) return CHOLAMD_ERR_ARG and say which
 * entry (cholamd_last_error) -- the conversion would turn it into inf or a denormal, which the pivot checks cannot be relied on to report.  Scale such a
 * matrix or use the fp64 factor, which has no such limit. */
int cholamd_device_fill_f32(cholamd_device *d, float *d_arena32, void *stream);
int cholamd_factor_f32(cholamd_device *d, float *d_arena32, void *stream);
int cholamd_factor_levels_f32(cholamd_device *d, float *d_arena32, int level_hi, int level_lo, void *stream);
int cholamd_solve_f32(cholamd_device *d, const float *d_arena32, const double *d_b, double *d_x, void *stream);
int cholamd_solve_refine(cholamd_device *d, const float *d_arena32, const double *d_b, double *d_x, int max_iter, double tol,
                         int *iters_out, double *relres_out, void *stream);
int cholamd_residual(cholamd_device *d, const double *d_b, const double *d_x, double *d_r, double *relres_out, void *stream);
/* ---- block solve (not in the reference, whose mmat.rg -b solves one vector): nrhs right-hand sides per pass over the factor.  B and X are column-major
 * n x nrhs fp64 device arrays in ORIGINAL dof order (column j at d_B + j * ldb / d_X + j * ldx, ldb, ldx >= n); rows n .. ld - 1 of X are never written.
 * X == B with ldx == ldb (in place) is allowed; any other overlap of X and B is undefined.  The right-hand sides are solved in chunks of 32 columns, each
 * one forward and one backward sweep over the solve lists of cholamd_solve (every stored entry of L read once per sweep per chunk, 16 x 32 fp64 MFMA tiles;
 * the off-diagonal blocks accumulate by fp64 atomics, so X agrees with cholamd_solve per column to rounding, not bit for bit); the 16x16 and span inverses are
 * formed once per call.  A chunk costs about the same for any number of columns up to 32: ~3 single solves with an fp64 factor, ~5 with an fp32 one, so
 * a chunk of fewer than 4 (fp64) / 6 (fp32) columns -- nrhs == 1 among them -- is solved column by column with the single-vector path instead.  Option
 * "solve_reference_shape" solves every column through cholamd_solve / cholamd_solve_f32, and so does option "solve_deterministic" (here and in
 * cholamd_solve_refine_nrhs: every column then has the bits of its single deterministic solve).
 * nrhs == 0 returns 0 and touches nothing; nrhs < 0, ldb < n, ldx < n or a NULL pointer with nrhs > 0: CHOLAMD_ERR_ARG.
 * cholamd_solve_nrhs / _f32 (fp64 / fp32 factor; vectors and arithmetic fp64) are asynchronous on `stream`.  cholamd_solve_refine_nrhs is
 * cholamd_solve_refine for every column (fp32 factor, residual in fp64 against the matrix file's A) and synchronises: chunk by chunk (the chunk's columns
 * of B are copied to a workspace first, so in-place use is allowed here too), corrections are applied to ALL columns of a chunk (converged columns are not
 * masked out) until every column has ||b_j - A x_j|| <= tol ||b_j|| or max_iter corrections have been applied; *iters_out = the most corrections any chunk
 * applied, relres_out[j] (nrhs doubles, may be NULL) = column j's final relative residual.  A NaN in any column fails as cholamd_solve_refine does
 * (CHOLAMD_ERR_ARG): the chunks after the failing one are not solved, their relres_out entries are NaN, *iters_out counts the chunks up to the failing one. */
int cholamd_solve_nrhs(cholamd_device *d, const double *d_arena, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, void *stream);
int cholamd_solve_nrhs_f32(cholamd_device *d, const float *d_arena32, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, void *stream);
int cholamd_solve_refine_nrhs(cholamd_device *d, const float *d_arena32, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, int max_iter,
                              double tol, int *iters_out, double *relres_out /* nrhs doubles, may be NULL */, void *stream);
/* ---- y = A x, and conjugate gradients preconditioned with the factor at hand (not in the reference).  A is the matrix with the values IN FORCE on the
 * device object: the plan's, or those of the last cholamd_device_set_values.  The factor in the arena may be that of OTHER values on the same pattern (the
 * previous Newton step's, the last time step's) or of lower precision (an fp32 arena): M = L L^T only has to be symmetric positive definite, and the loop
 * solves A x = b with the values in force to `tol` in a number of steps set by the spectrum of M^-1 A -- one where A = c M, m + 1 after a change of rank m,
 * a handful for a drift of a few per cent -- where the stationary iteration of cholamd_solve_refine may diverge (A = 3 M: iteration matrix -2 I).
 *   cholamd_apply / _nrhs: y = A x (vectors in original dof order; blocks column-major with leading dimensions >= n, rows n .. ld - 1 never written), per row
 *     acc = fma(a_ie, x_e, acc) over the row's entries in the order of the plan's CSR from 0.0; asynchronous; y overlapping x: CHOLAMD_ERR_ARG.
 *     cholamd_plan_apply_host is the same order on the host (bit for bit); values == NULL: the plan's values, otherwise a value array of cholamd_plan_nz()
 *     doubles as cholamd_device_set_values takes it (entries that were explicit zeros when the plan was made are not part of the operator).
 *   cholamd_solve_pcg / _f32 / _nrhs / _nrhs_f32: standard PCG, M^-1 = what cholamd_solve / _f32 (the one-vector forms) or cholamd_solve_nrhs / _f32 run under
 *     the options in force.  Start: x = 0, r = b; flags = CHOLAMD_PCG_X0: the caller's x, r = b - A x.  b is copied to a workspace first: x == b is allowed.
 *     A column claims convergence when the recurrence's ||r||^2 <= tol^2 ||b||^2; the TRUE residual b - A x is then formed, and if ||b - A x|| <= tol ||b||
 *     the column ends (status 0); otherwise the true residual replaces r, p = M^-1 r, and the column runs on (that step counts as no iteration).
 *     Outputs per column (HOST arrays of nrhs entries, one entry in the one-vector forms; each may be NULL): iters = applications of A to p, relres = the TRUE
 *     ||b - A x|| / ||b|| of the x returned, status = 0 converged | 1 max_iter reached (return code 0, as for the refinement) | 2 breakdown: p^T A p <= 0
 *     or r^T M^-1 r <= 0 -- the values in force are not positive definite, or the factor is broken; x keeps the last iterate | 3 NaN or inf.  Status 2 or 3
 *     in any column: CHOLAMD_ERR_ARG after ALL columns have been worked on, cholamd_last_error names the first such column and the quantity.  b = 0: x = 0,
 *     0 iterations, relres 0, status 0.  The calls synchronise `stream` once per iteration (one read-back of the columns' states); every scalar of the
 *     iteration stays in device memory.  Workspaces (five n x 32 blocks, partial sums, the records) belong to the device object and are allocated at the
 *     first call; ONE CALL AT A TIME per device object.  The blocks have their full width of 32 columns whatever nrhs is, the one-vector forms included (with
 *     the residual block they share with cholamd_solve_refine_nrhs: 6 * 32 * 8 n bytes, 1.5 GB at n = 10^6), so that no later call allocates; cholamd_apply /
 *     _nrhs need the CSR operator alone.  A column that has finished stays in its chunk's launches until the chunk ends (alpha = beta = 0 select no write):
 *     a chunk costs what its slowest column costs.
 *     Arguments: those of cholamd_solve_nrhs (nrhs == 0 returns 0 and touches nothing; nrhs < 0, a small ld, a NULL pointer with nrhs > 0: CHOLAMD_ERR_ARG),
 *     unknown flags, tol negative or not finite: CHOLAMD_ERR_ARG, nothing written.  Columns go in chunks of 32; a chunk's loop ends when none of its columns runs.
 *     SCOPE: the complete factor -- a single-GPU device object, or rank 0 after a gather; another rank of a partitioned object: CHOLAMD_ERR_ARG.  Follow-ups,
 *     not here: low-rank objects (cholamd_lowrank_*), the sharded and multi-rank forms, autograd.
 *   BITS.  The vector kernels have one owner per element, no atomics, and sum in a fixed order, so the loop is as reproducible as the solve inside it:
 *     (a) option solve_deterministic: two calls return the same iters, relres, status and bits of x;
 *     (b) solve_deterministic without solve_deterministic_block: column j of an _nrhs call has the bits and the iteration count of the one-vector call on it;
 *     (c) both options: column j depends on column j of B alone (and of X under CHOLAMD_PCG_X0) -- not on nrhs, on its chunk, or on a NaN next to it;
 *     (d) on the atomic solve paths nothing is promised beyond the tolerances. */
#define CHOLAMD_PCG_X0 1
int cholamd_apply(cholamd_device *d, const double *d_x, double *d_y, void *stream);
int cholamd_apply_nrhs(cholamd_device *d, const double *d_X, int64_t ldx, double *d_Y, int64_t ldy, int nrhs, void *stream);
int cholamd_plan_apply_host(const cholamd_plan *p, const double *values /* or NULL */, const double *x, double *y);
int cholamd_solve_pcg(cholamd_device *d, const double *d_arena, const double *d_b, double *d_x, int max_iter, double tol, int flags,
                      int *iters_out, double *relres_out, int *status_out, void *stream);
int cholamd_solve_pcg_f32(cholamd_device *d, const float *d_arena32, const double *d_b, double *d_x, int max_iter, double tol, int flags,
                          int *iters_out, double *relres_out, int *status_out, void *stream);
int cholamd_solve_pcg_nrhs(cholamd_device *d, const double *d_arena, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, int max_iter, double tol, int flags,
                           int *iters_out, double *relres_out, int *status_out, void *stream);
int cholamd_solve_pcg_nrhs_f32(cholamd_device *d, const float *d_arena32, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, int max_iter, double tol, int flags,
                               int *iters_out, double *relres_out, int *status_out, void *stream);
/* ---- one triangular half of the solve, the factor's diagonal and log det A (not in the reference; CHOLMOD's CHOLMOD_L / CHOLMOD_Lt systems and the logdet
 * every sparse Cholesky offers).  THE SQUARE ROOT these calls speak about is M = P^T L P in ORIGINAL dof order (P the plan's permutation, L the factor in
 * the arena): M M^T = A, A^-1 = M^-T M^-1, and no caller ever sees permuted coordinates.  M y = b whitens b (b^T A^-1 b = ||y||^2); M^T x = z turns white
 * noise z into a sample x ~ N(0, A^-1).
 * cholamd_solve_half / _f32 (fp64 / fp32 factor; vectors and arithmetic fp64): x = M^-1 b (which = CHOLAMD_HALF_FORWARD) or x = M^-T b
 * (CHOLAMD_HALF_BACKWARD), b and x n doubles on the device in original dof order, asynchronous on `stream`; d_x == d_b is allowed (as in cholamd_solve, b is
 * permuted into the work vector first).  Each is the permute, that sweep's launches of cholamd_solve, and the permute back: BACKWARD(FORWARD(b)) is the
 * solve and agrees with cholamd_solve to rounding (atomics in the off-diagonal blocks: not bit for bit; bit for bit under option "solve_deterministic").  The 16x16 and 256-column span inverses are formed
 * from d_arena at the start of EVERY half call (as at the start of a solve): a BACKWARD call does not rely on a preceding FORWARD call, whose arena may have
 * been another.  Option "solve_reference_shape" selects the deterministic per-call kernels for the halves of an fp64 factor as it does for cholamd_solve;
 * option "solve_deterministic" selects the deterministic streamed sweeps for the halves of either factor (the _nrhs forms then go column by column).
 * cholamd_solve_half_nrhs / _f32: the same for nrhs columns, with the argument rules of cholamd_solve_nrhs verbatim (column-major n x nrhs, ldb, ldx >= n,
 * rows n .. ld - 1 of X never written, in place with X == B and ldx == ldb; nrhs == 0 returns 0 and touches nothing; nrhs < 0, ldb < n, ldx < n or a NULL
 * pointer with nrhs > 0: CHOLAMD_ERR_ARG), the 32-column chunks and kernels of cholamd_solve_nrhs with one sweep instead of two, the inverses once per
 * call, and the same small-chunk rule: a chunk of fewer than 4 (fp64) / 6 (fp32) columns is solved column by column; column j agrees with
 * cholamd_solve_half of column j to rounding.
 * `which` other than 0 / 1: CHOLAMD_ERR_ARG, nothing written.
 * cholamd_factor_logdet / _f32: *logdet_out (HOST) = log det A = 2 sum_i log L_ii, accumulated in fp64 (an fp32 factor's diagonal is converted before the
 * log).  Synchronises `stream` (it returns a host scalar, like cholamd_residual).  DETERMINISTIC: a fixed assignment of entries to lanes, one partial sum
 * per workgroup, the partials summed in a fixed order by a second one-workgroup launch (every addition error-free: the sum is carried as a pair of doubles); no floating-point atomics anywhere, so two calls on
 * the same arena return the same bits.  A diagonal entry that is not a positive finite number (a failed or never-run factorisation, a poisoned arena)
 * makes the call return CHOLAMD_ERR_ARG with *logdet_out = NaN; cholamd_last_error() names the separator and (1-based) column of the first such entry in
 * permuted order -- the smallest position, an integer minimum independent of the order in which workgroups finish.
 * cholamd_factor_diag / _f32: d_diag[dof] = L(p, p) with p the permuted position of dof (n doubles on the device, asynchronous on `stream`): the diagonal
 * of M; 2 sum log d_diag equals the logdet to summation rounding.
 * All eight need the COMPLETE factor in the arena: a single-GPU device object, or rank 0's after cholamd_gather_to_root / cholamd_gather_factor (they use
 * the solve lists of the whole tree, like cholamd_solve on a partitioned device).  There are no sharded variants. */
#define CHOLAMD_HALF_FORWARD  0   /* x = M^-1 b   = P^T L^-1 P b   */
#define CHOLAMD_HALF_BACKWARD 1   /* x = M^-T b   = P^T L^-T P b   */
int cholamd_solve_half(cholamd_device *d, const double *d_arena, const double *d_b, double *d_x, int which, void *stream);
int cholamd_solve_half_f32(cholamd_device *d, const float *d_arena32, const double *d_b, double *d_x, int which, void *stream);
int cholamd_solve_half_nrhs(cholamd_device *d, const double *d_arena, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, int which, void *stream);
int cholamd_solve_half_nrhs_f32(cholamd_device *d, const float *d_arena32, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, int which, void *stream);
int cholamd_factor_logdet(cholamd_device *d, const double *d_arena, double *logdet_out, void *stream);
int cholamd_factor_logdet_f32(cholamd_device *d, const float *d_arena32, double *logdet_out, void *stream);
int cholamd_factor_diag(cholamd_device *d, const double *d_arena, double *d_diag, void *stream);
int cholamd_factor_diag_f32(cholamd_device *d, const float *d_arena32, double *d_diag, void *stream);
/* ---- the factor applied FORWARDS (not in the reference): y = M z, y = M^T z and y = M M^T z with the square root M = P^T L P of the half solves above, so
 * cholamd_multiply_half(which) is the inverse of cholamd_solve_half(which).  x = M z turns white noise z into a sample x ~ N(0, A) (A a sparse
 * covariance; the mirror of the N(0, A^-1) sample of CHOLAMD_HALF_BACKWARD); ||M^T x||^2 = x^T A x is the energy norm; ||A z - M M^T z|| / ||A z|| says
 * whether an arena still factors the CURRENT values of A, and how well.
 * cholamd_multiply_half / _f32 (fp64 / fp32 factor; vectors and arithmetic fp64, an fp32 factor is converted on load): y = M z = P^T L P z
 * (which = CHOLAMD_HALF_FORWARD) or y = M^T z = P^T L^T P z (CHOLAMD_HALF_BACKWARD), z and y n doubles on the device in original dof order, asynchronous
 * on `stream`; d_y == d_z is allowed (z is permuted into the device object's work vector first).  Input and output of a product are distinct vectors, so
 * there is no leaf-to-root chain: after the permute ONE launch covers the whole tree and reads every stored entry of L it needs once -- the lower triangles
 * of the diagonal blocks (the upper triangles are not part of the factor and are never read) and the stored row runs of the panels; the structural zeros of
 * the leaf panels that the solve skips (cholamd_plan_solve_skips) are skipped here too.
 * cholamd_multiply / _f32: y = M M^T z, the BACKWARD product followed by the FORWARD product in permuted coordinates (the permutation applied once on the
 * way in and once on the way out, the intermediate vector belongs to the device object): three launches.
 * DETERMINISTIC: every element of y has ONE owner -- a 16-row chunk of a separator gathers its rows from the separator's diagonal block and from the
 * panels of its descendants in a fixed order (FORWARD), a 16-column chunk of a separator sums over its own columns of the panel (BACKWARD) -- and a fixed
 * summation order; no floating-point atomics anywhere: two calls on one arena and one input return the same bits (unlike the streamed solve without option "solve_deterministic").
 * cholamd_multiply_half_nrhs / cholamd_multiply_nrhs / _f32: the same products for the nrhs columns of Z, Y = M Z, M^T Z or M M^T Z.  Z and Y are column-major
 * n x nrhs on the device in original dof order with leading dimensions ldz, ldy >= n (rows n .. ld - 1 of Y are never written), the argument rules those of
 * cholamd_solve_half_nrhs: Y == Z with ldy == ldz is allowed (a chunk is permuted into the workspace before anything is written), nrhs == 0 returns 0 and
 * touches nothing, nrhs < 0, a small ld or a NULL pointer with nrhs > 0 is CHOLAMD_ERR_ARG; and those of the products: a bad `which`, a Y (its
 * (nrhs - 1) ldy + n doubles) that overlaps the arena, another rank of a partitioned object are CHOLAMD_ERR_ARG.  The columns go in chunks of 32: a chunk is
 * permuted into a row-major block and ONE launch per direction walks the same owner lists with 16 x 32 v_mfma_f64_16x16x4_f64 tiles, so every stored entry of
 * L is read once per chunk, not once per column; the last launch writes Y in original dof order itself.  The same determinism: one owner per element, the
 * four partial tiles of a workgroup added in a fixed order, no floating-point atomics.  Within ONE column a NaN or inf of z reaches the whole 16-position
 * tile of a diagonal block it belongs to (an entry above the diagonal is an operand 0.0 of the tile product, and 0 * inf is NaN); other columns never see
 * it.  A chunk of fewer columns than a measured threshold goes column by column through the single-vector products (device option "multiply_nrhs_min",
 * CHOLAMD_MULTIPLY_NRHS_MIN at cholamd_device_create: 1 = every chunk takes the block kernel, 33 = none does, <= 0 = the measured default).  The two n x 32
 * blocks are allocated at the first chunk that takes the block kernel; later calls allocate nothing.  Asynchronous on `stream`.
 * cholamd_plan_multiply_host_nrhs: the block product on the HOST (which = 0, 1, or -1: the full product) with the block kernel's own partition of a source
 * (chol_plan.h at chol_muln_wave); the same argument rules.
 * `which` other than 0 / 1, a NULL pointer, or a result that overlaps the arena: CHOLAMD_ERR_ARG, nothing written.
 * cholamd_factor_residual / _f32: *rel_out (HOST) = ||A z - M M^T z||_2 / ||A z||_2 for the probe z (n doubles on the device, original dof order), A z from the
 * device object's residual operator, which holds the CURRENT values (as cholamd_residual uses them after cholamd_device_set_values): two passes over L and one
 * over A, all on the device.  Synchronises `stream`.  The two norms are reduced deterministically: one partial pair per workgroup by plain stores, summed in a
 * fixed order by a second one-workgroup launch (the scheme of cholamd_factor_logdet), no atomics -- two calls return the same double.  A NaN or inf anywhere
 * (z, A's values, the arena) gives CHOLAMD_ERR_ARG with *rel_out = NaN, as cholamd_solve_refine treats it.
 * All of them need the COMPLETE factor in the arena, like the half solves: a single-GPU device object, or rank 0's after a gather; another rank of a
 * partitioned object returns CHOLAMD_ERR_ARG.  There are no sharded variants.  ONE CALL AT A TIME per device object: the work vector, the second vector of
 * cholamd_multiply and the lists (built and uploaded at the first call; later calls allocate nothing) belong to the object.
 * cholamd_plan_multiply_host: the same product on the HOST over a host arena (tests and diagnostics, no device): it walks the SAME owner lists -- the same
 * owner assignment, the lower triangles only, row compaction honoured; z and y n doubles in original dof order, y == z allowed.  It builds the lists
 * anew at every call (a diagnostic, not a hot path).
 * cholamd_plan_multiply_counts: the size of those lists, out = { FORWARD items, FORWARD sources, entries of L a FORWARD product reads, BACKWARD items,
 * BACKWARD sources, entries a BACKWARD product reads } (an entry is 8 bytes of an fp64 arena, 4 of an fp32 one; a source is 24 bytes of list). */
int cholamd_multiply_half(cholamd_device *d, const double *d_arena, const double *d_z, double *d_y, int which, void *stream);
int cholamd_multiply_half_f32(cholamd_device *d, const float *d_arena32, const double *d_z, double *d_y, int which, void *stream);
int cholamd_multiply(cholamd_device *d, const double *d_arena, const double *d_z, double *d_y, void *stream);
int cholamd_multiply_f32(cholamd_device *d, const float *d_arena32, const double *d_z, double *d_y, void *stream);
int cholamd_factor_residual(cholamd_device *d, const double *d_arena, const double *d_z, double *rel_out, void *stream);
int cholamd_factor_residual_f32(cholamd_device *d, const float *d_arena32, const double *d_z, double *rel_out, void *stream);
int cholamd_multiply_half_nrhs(cholamd_device *d, const double *d_arena, const double *d_Z, int64_t ldz, double *d_Y, int64_t ldy, int nrhs, int which, void *stream);
int cholamd_multiply_half_nrhs_f32(cholamd_device *d, const float *d_arena32, const double *d_Z, int64_t ldz, double *d_Y, int64_t ldy, int nrhs, int which, void *stream);
int cholamd_multiply_nrhs(cholamd_device *d, const double *d_arena, const double *d_Z, int64_t ldz, double *d_Y, int64_t ldy, int nrhs, void *stream);
int cholamd_multiply_nrhs_f32(cholamd_device *d, const float *d_arena32, const double *d_Z, int64_t ldz, double *d_Y, int64_t ldy, int nrhs, void *stream);
int cholamd_plan_multiply_host(const cholamd_plan *p, const double *arena_host, int which, const double *z, double *y);
int cholamd_plan_multiply_host_nrhs(const cholamd_plan *p, const double *arena_host, int which, const double *Z, int64_t ldz, double *Y, int64_t ldy, int nrhs);
int cholamd_plan_multiply_counts(const cholamd_plan *p, int64_t out[6]);
/* ---- selected inversion (not in the reference; the Takahashi recursion every sparse Cholesky package offers): the entries of A^-1 on the pattern of the
 * factor -- the diagonal of A^-1 (marginal variances of a Gaussian Markov random field, leverage scores), the entries on the pattern of A (the trace term
 * tr(A^-1 dA) of a likelihood gradient) -- from the factor, in a small multiple of the factorisation's flops instead of n solves.  fp64 factor only.
 * With Z = (P A P^T)^-1 = L^-T L^-1 and, for the columns J of a separator, "below" = the rows its panel stores after them:
 *   Y = L[below, J] L[J, J]^-1,   Z[below, J] = -Z[below, below] Y,   Z[J, J] = L[J, J]^-T L[J, J]^-1 - Y^T Z[below, J],
 * root first, in column blocks of CHOLAMD_SELINV_BLOCK columns, last block first; Z[below, below] is read from the panels of the ancestors (and the later
 * blocks), which are complete by then.
 * cholamd_selinv: d_zarena = cholamd_plan_arena_doubles() doubles in device memory with THE ARENA'S OWN LAYOUT: the element that holds L(i, j) in d_arena
 * holds Z(i, j) in d_zarena (lower triangle in the diagonal blocks); cholamd_plan_arena_to_dense and cholamd_plan_region read it like a factor.
 * Asynchronous on `stream`.  Every element of d_zarena is written by the call, whatever it held before (the call starts by zeroing it).
 * WHAT IS EXACT: the positions of the structural pattern of L (every position where L can be non-zero, hence every position of tril(P A P^T)).  Stored
 * positions outside that pattern (the rest of the 16-row tiles a panel stores, the parent's rows, the upper triangles and padding rows: zero) hold
 * finite numbers without meaning for a finite factor.  A position of Z[below, below] no panel stores reads as 0.0: it only ever meets an exact zero of Y.
 * DETERMINISTIC: every element has one owner and a fixed summation order, no floating-point atomics: two calls on one factor return the same bits.
 * d_zarena overlapping d_arena (d_zarena == d_arena included): CHOLAMD_ERR_ARG, nothing written -- there is no in-place form.  A NULL pointer:
 * CHOLAMD_ERR_ARG.  The first call on a device object builds and uploads the gather lists and allocates the workspace (two row-major strips of 64 doubles
 * per panel row of the widest level); later calls allocate nothing.  A failed factorisation (cholamd_factor_info != 0) gives numbers without meaning (inf
 * and NaN among them), never a hang.  Like the calls above it needs the COMPLETE factor: a single-GPU device object, or rank 0's after a gather; on
 * another rank of a partitioned object it returns CHOLAMD_ERR_ARG (that the gather has happened on rank 0 is the caller's business, as for cholamd_solve).
 * ONE CALL AT A TIME per device object: the workspace (and the lists, built at the first call) belong to the object, as the factorisation's and the
 * solve's do (see cholamd_factor) -- order the cholamd_selinv calls of one object on one stream, or use one object per concurrent stream.
 * cholamd_selinv_diag and cholamd_selinv_entries use no workspace.
 * cholamd_selinv_diag: d_diag[dof] = (A^-1)(dof, dof), n doubles on the device in original dof order, asynchronous: cholamd_factor_diag's walk (the same
 * kernel) over the Z arena.
 * cholamd_selinv_entries: the mirror image of cholamd_device_set_values -- d_vals[k] = (A^-1)(row_k, col_k) for entry k of the plan's entry list
 * (cholamd_plan_entries: the VALUE-ARRAY order), count = cholamd_plan_nz() doubles on the device, asynchronous.  Entries outside the pattern (0.0 when the
 * plan was made) or dropped by the ordering have no position in any arena: they are written as quiet NaN.  Duplicate entries of one position all receive
 * the value.  count != cholamd_plan_nz() or a NULL pointer: CHOLAMD_ERR_ARG, nothing written.
 * Host view of the gather lists (tests and diagnostics, no device): cholamd_plan_selinv_blocks = column blocks of separator `sep` (label);
 * cholamd_plan_selinv_front: for column block `block` of `sep`, cols[0] = permuted position of the block's first column, cols[1] = its columns; returns m =
 * the rows below it; pos[i], i < m = their permuted positions (ascending); off[i * m + j] = the Z-arena offset the kernels read Z(pos[i], pos[j]) from
 * (symmetric: the stored side) or -1 = not stored, read as 0.0.  pos and off may be NULL (the count alone).  The offset table is quadratic in m: with pos or
 * off given, m > cap or m > CHOLAMD_SELINV_FRONT_MAX is refused (CHOLAMD_ERR_ARG) -- not a call for the fronts of a large problem. */
#define CHOLAMD_SELINV_BLOCK 64
#define CHOLAMD_SELINV_FRONT_MAX 8192
int cholamd_selinv(cholamd_device *d, const double *d_arena, double *d_zarena, void *stream);
int cholamd_selinv_diag(cholamd_device *d, const double *d_zarena, double *d_diag, void *stream);
int cholamd_selinv_entries(cholamd_device *d, const double *d_zarena, double *d_vals, int64_t count, void *stream);
int cholamd_plan_selinv_blocks(const cholamd_plan *p, int sep);
int cholamd_plan_selinv_front(const cholamd_plan *p, int sep, int block, int cap, int cols[2], int *pos, int64_t *off);
/* ---- gradients with respect to the value array (not in the reference): the contraction of an adjoint onto the entries of A, for callers who hold the value
 * array of cholamd_device_set_values as the variable of an optimisation.  The matrix is the linear function of the value array v that the residual operator
 * implements,  A(v) = sum_k v_k E_k,  E_k = e_i e_j^T + e_j e_i^T for an off-diagonal entry k at (i, j) = (row_k, col_k) of cholamd_plan_entries and
 * E_k = e_i e_i^T for a diagonal one: multiplicity m_k = 2 off the diagonal, 1 on it.  Both calls compute  g[k] = alpha s_k + beta g[k]  for every k:
 *   cholamd_values_grad_pairs:   s_k = sum_c p_c^T E_k q_c = sum_c (P[i, c] Q[j, c] + P[j, c] Q[i, c])  (sum_c P[i, c] Q[i, c] on the diagonal), P and Q
 *     column-major n x nrhs on the device in original dof order, ldp, ldq >= n.  With X = A^-1 B and Lam = A^-1 (dloss / dX) the gradient of the loss with
 *     respect to v is the call with P = Lam, Q = X, alpha = -1; d_P == d_Q is allowed (alpha = 1: d(x^T A x) / dv).
 *   cholamd_values_grad_logdet:  s_k = tr(A^-1 E_k) = m_k (A^-1)(i, j) = d(log det A) / dv_k, read from the Z arena of cholamd_selinv.
 * Entries outside the pattern (0.0 when the plan was made) are ignored by everything the library computes, so their derivative is zero: s_k = 0, they
 * receive beta g[k] -- never NaN.  beta == 0: g is not read (g[k] = alpha s_k; 0.0 outside the pattern), so a NaN-filled or uninitialised g comes out finite.
 * THE ORDER OF THE SUM is part of the contract: acc = 0; for c = 0 .. nrhs - 1: acc = fma(P[i, c], Q[j, c], acc), then, off the diagonal,
 * acc = fma(P[j, c], Q[i, c], acc); g = beta == 0 ? alpha acc : fma(alpha, acc, beta g).  One owner per entry, no atomics: the same bits every call, and
 * the bits of the host restatements below.
 * REFUSED PLANS (CHOLAMD_ERR_ARG, the message names the first offending entry): a plan with cholamd_plan_dropped_entries() > 0 (the arena does not factor
 * A) and a plan with cholamd_plan_duplicate_entries() > 0 -- two in-pattern entries at one position: the scatter overwrites where the residual operator
 * sums, so A(v) is not the sum above.  cholamd_plan_duplicate_entries: the in-pattern entries that repeat the position of another one, counted when the
 * plan is made.
 * Both device calls are asynchronous on `stream`.  nrhs == 0 returns 0 and touches nothing.  CHOLAMD_ERR_ARG with nothing written: count !=
 * cholamd_plan_nz(), a NULL pointer, nrhs < 0, ldp < n or ldq < n, d_g overlapping P, Q (their full extents (nrhs - 1) ld + n) or the Z arena, a
 * partitioned device object (world > 1).  The first call on a device object uploads the entry list; later calls allocate nothing.  fp64 only.
 * cholamd_plan_values_grad_pairs_host / _logdet_host: the same on the CPU with host arrays (zarena_host: a host copy of the Z arena), walking the same lists
 * in the same order with fma(): the device's bits. */
int cholamd_values_grad_pairs(cholamd_device *d, const double *d_P, int64_t ldp, const double *d_Q, int64_t ldq, int nrhs,
                              double alpha, double beta, double *d_g, int64_t count, void *stream);
int cholamd_values_grad_logdet(cholamd_device *d, const double *d_zarena, double alpha, double beta, double *d_g, int64_t count, void *stream);
int cholamd_plan_values_grad_pairs_host(const cholamd_plan *p, const double *P, int64_t ldp, const double *Q, int64_t ldq, int nrhs,
                                        double alpha, double beta, double *g, int64_t count);
int cholamd_plan_values_grad_logdet_host(const cholamd_plan *p, const double *zarena_host, double alpha, double beta, double *g, int64_t count);
int64_t cholamd_plan_duplicate_entries(const cholamd_plan *p);
/* ---- Schur complement on the top of the tree, with condense and expand (not in the reference; the "Schur complement" / "partial factorisation" option of
 * MUMPS and PARDISO): eliminate the interior dofs I, keep the interface dofs T, and receive  S = A_TT - A_TI A_II^-1 A_IT  -- substructuring, domain
 * decomposition, static condensation, constrained Gaussian Markov random fields.  The caller assembles or solves the interface problem, then recovers the interior.
 * k = the number of tree levels KEPT, 1 <= k <= levels - 1: the kept separators are heap indices 1 .. 2^k - 1 (cholamd_plan_tree), m = the sum of their sizes,
 * t0 = n - m.  They are the tail [t0, n) of the permuted order (checked: CHOLAMD_ERR_INVARIANT otherwise).
 * THE SCHUR ORDER: entry i of every m-vector and row / column i of S is permuted position t0 + i, i.e. original dof perm[t0 + i] (cholamd_plan_schur_dofs).
 * Why the arena holds S: the factorisation is right-looking and level by level, leaves first.  After the levels levels - 1 .. k every contribution of the
 * eliminated separators has been extend-added into the blocks of the kept ones, and nothing else has touched them: they hold S, lower triangle, in the arena's
 * row-compacted layout.
 *
 * Host side (no device):
 * cholamd_plan_schur_size: m, or CHOLAMD_ERR_ARG for k out of range.
 * cholamd_plan_schur_dofs: writes the m original dof ids in Schur order, returns m.
 * cholamd_plan_schur_list (tests and diagnostics): one record of CHOLAMD_SCHUR_RECORD int64 per STORED 16-row tile piece of a block of two kept separators:
 *   [0] arena offset of the piece's first element, [1] leading dimension, [2] rows (<= 16), [3] columns, [4] first row and [5] first column in Schur
 *   coordinates, [6] 1 = the piece lies in a diagonal block, which stores its lower triangle: only elements with row >= column are meant (its columns end at the
 *   tile's last row).  Element (i, j) of a piece is arena[[0] + i + j * [1]] = S([4] + i, [5] + j).  Lower-triangle positions of S no record covers are exact
 *   zeros: the two separators are not ancestor and descendant, or the row compaction dropped the tile (cholamd_plan_block_tile_map: -1).  Returns the number of
 *   records and writes at most cap of them; cap = 0 (out may be NULL) sizes the buffer.  The gather kernel's list is built from the same enumeration (cut into
 *   chunks of 64 columns, the pieces without storage added as zeros).
 * cholamd_plan_schur_host: the gather restated on the CPU over a host arena: S column-major m x m, lds >= m, both triangles, every element written, rows
 *   m .. lds - 1 untouched.  NULL pointer or lds < m: CHOLAMD_ERR_ARG, nothing written.
 *
 * Device side.  Common rules -- CHOLAMD_ERR_ARG with NOTHING written for: k out of range, a NULL pointer, a partitioned device object (world > 1).  There are
 * NO sharded variants of these calls.  Condense and expand have block forms for many right-hand sides (cholamd_schur_condense_nrhs, below).
 * cholamd_schur_factor: eliminates the levels levels - 1 .. k of a filled arena by the per-level launches -- the launches of cholamd_factor_levels(d, a,
 *   levels - 1, k); it never uses the one-launch program, whatever the problem's size.  Asynchronous on `stream`; cholamd_factor_info reports pivots as usual.
 *   cholamd_factor_levels(d, a, k - 1, 0) afterwards COMPLETES the factor: the arena is then bit-identical to one factored by cholamd_factor_levels(d, a,
 *   levels - 1, 0).
 * cholamd_schur: d_S column-major m x m in device memory, lds >= m, BOTH triangles (the stored lower one is mirrored).  Every one of the m x m elements is
 *   written by the call -- the exact zeros between unrelated kept separators and of tiles without storage included; rows m .. lds - 1 are never touched.  A pure
 *   gather: one owner per element, no atomics, bit-identical from call to call.  Asynchronous.  lds < m, or d_S overlapping the arena: CHOLAMD_ERR_ARG.  The
 *   piece list is uploaded at the first call per (device object, k); later calls allocate nothing.  fp64 arena ONLY: there is no cholamd_schur_f32 (take S from
 *   an fp64 run).
 * cholamd_schur_condense: d_b n doubles in ORIGINAL dof order; d_g m doubles in Schur order = b_T - A_TI A_II^-1 b_I; d_w n doubles of opaque state for the
 *   expand (the permuted, forward-swept vector).  The call permutes, forms the 16x16 and span inverses of the levels >= k ONLY -- the levels < k hold S, not a
 *   factor, and are never read as one -- and runs the forward sweep of the levels levels - 1 .. k with the kernels of cholamd_solve.  The off-diagonal blocks
 *   accumulate by fp64 atomics: g agrees from run to run to rounding, not bit for bit (unless option "schur_deterministic" is set, below).  Asynchronous.  b, w, g and the arena must not overlap each other:
 *   CHOLAMD_ERR_ARG.
 * cholamd_schur_expand: d_xt = the caller's solution of S x_T = g (m doubles, Schur order); d_x = the full solution, n doubles, original order.  Backward sweep
 *   of the levels k .. levels - 1 and the inverse permutation.  d_w is NOT modified (the sweep runs in the device object's work vector, and the inverses are
 *   formed again from d_arena, as at the start of every half solve), so one condense serves any number of expands.  x overlapping w, xt or the arena:
 *   CHOLAMD_ERR_ARG.  ONE CALL AT A TIME per device object, as for the solve.  Asynchronous.
 * _f32: the same on an fp32 arena partially factored with cholamd_factor_levels_f32(d, a32, levels - 1, k) (vectors and arithmetic fp64).
 * A failed factorisation (cholamd_factor_info != 0) gives numbers without meaning, never a hang. */
#define CHOLAMD_SCHUR_RECORD 7
int cholamd_plan_schur_size(const cholamd_plan *p, int k);
int cholamd_plan_schur_dofs(const cholamd_plan *p, int k, int *dofs_out);
int cholamd_plan_schur_list(const cholamd_plan *p, int k, int64_t cap, int64_t *out);
int cholamd_plan_schur_host(const cholamd_plan *p, int k, const double *arena_host, double *S, int64_t lds);
int cholamd_schur_factor(cholamd_device *d, double *d_arena, int k, void *stream);
int cholamd_schur(cholamd_device *d, const double *d_arena, int k, double *d_S, int64_t lds, void *stream);
int cholamd_schur_condense(cholamd_device *d, const double *d_arena, int k, const double *d_b, double *d_w, double *d_g, void *stream);
int cholamd_schur_expand(cholamd_device *d, const double *d_arena, int k, const double *d_w, const double *d_xt, double *d_x, void *stream);
int cholamd_schur_condense_f32(cholamd_device *d, const float *d_arena32, int k, const double *d_b, double *d_w, double *d_g, void *stream);
int cholamd_schur_expand_f32(cholamd_device *d, const float *d_arena32, int k, const double *d_w, const double *d_xt, double *d_x, void *stream);
/* ---- Schur condense / expand for many right-hand sides, and the bit-reproducible form of all of them.
 * cholamd_schur_condense_nrhs / cholamd_schur_expand_nrhs (and _f32: an fp32 arena eliminated with cholamd_factor_levels_f32(d, a32, levels - 1, k)):
 *   B, X   n x nrhs column-major in ORIGINAL dof order, ldb, ldx >= n
 *   W      n x nrhs column-major, ldw >= n: column j is what cholamd_schur_condense writes as w for column j of B (the permuted, forward-swept vector, whose
 *          tail is g).  A column of W is a valid w for cholamd_schur_expand, and a w is a valid column of W.
 *   G, XT  m x nrhs column-major in Schur order, ldg, ldxt >= m
 * NEVER WRITTEN: rows past n (m) up to the leading dimension, columns >= nrhs, and W by the expand (one condense serves any number of expands).
 * nrhs == 0 returns 0 and touches nothing; nrhs < 0, a leading dimension that is too small, or a NULL pointer with nrhs > 0: CHOLAMD_ERR_ARG, nothing written;
 * so for k out of range and a partitioned device object.  Condense: B, W, G and the arena must be pairwise disjoint over their full (nrhs - 1) ld + rows
 * extents; expand: X must be disjoint from W, XT and the arena; there is no in-place form.  Asynchronous on `stream`; ONE CALL AT A TIME per device object.
 * The columns go in chunks of 32 through the device object's permuted row-major block: the 16x16 and span inverses of the levels >= k ONLY are formed once per
 * call, the condense runs the forward loop of the block solve over the levels levels - 1 .. k and unpacks the block into W and G, the expand packs W's rows
 * < t0 and XT into the block and runs the backward loop over k .. levels - 1.  A chunk of fewer than 4 (fp64 arena) / 6 (fp32 arena) columns goes column
 * by column through the single-vector calls.  The off-diagonal blocks accumulate by fp64 atomics: results agree from run to run to rounding.
 *
 * DEVICE OPTION "schur_deterministic" (cholamd_device_set_option, or CHOLAMD_SCHUR_DETERMINISTIC non-zero in the environment at cholamd_device_create;
 * default off; setting it rebuilds nothing).  With it off every entry point does exactly what it does without it, down to which kernels run -- the Schur
 * sweeps under "solve_deterministic" included.  It does not depend on the solve_* options and does not change them.  With it on, cholamd_schur_condense /
 * _expand / _f32 walk deterministic step lists CUT at level k with the gather and span kernels of the deterministic solve, and the four _nrhs calls walk the
 * same lists on 32-column chunks with the block gather and the block span kernel in its substitution form; EVERY chunk takes the block kernels, whatever
 * its column count, nrhs = 1 included.  No floating-point atomic, no flag, no wait inside a launch.  The lists are built per (device object, k) at the
 * first such call and kept; later calls allocate nothing:
 *   FORWARD (condense)  the FORWARD steps of the deterministic solve of the levels levels - 1 .. k, unchanged, then ONE kept lead step: for every 16-row
 *                       chunk of every kept separator the sources of its ordinary lead-step item that read permuted positions < t0 (the panels of its
 *                       eliminated descendants).  Sources in panels of kept separators are dropped: those hold S, not L.  One launch, no span step.
 *   BACKWARD (expand)   the BACKWARD steps of the levels k .. levels - 1, unchanged: their sources into kept ancestors are rows L[T, s] of eliminated panels.
 * The builder refuses (CHOLAMD_ERR_INVARIANT, naming the item) a list in which a kept-lead source reads a position >= t0, a source lies in a block of two
 * kept separators, a position under the cut is not solved exactly once, or a kept position has more than one owner.  The 16x16 inverses are formed for the
 * levels >= k only.  THE CONTRACT with the option on:
 *  (a) the same bits of W, G and X for the same arena and inputs -- from call to call, between device objects of one plan, and on a device object created
 *      under CHOLAMD_POISON=1;
 *  (b) in the _nrhs forms column j depends on the arena and on column j of the inputs only -- not on nrhs, not on its chunk or its half of the 32-column
 *      tile, not on the other columns: a NaN elsewhere never reaches it;
 *  (c) nothing stored in a block of two kept separators influences any output: condense and expand never read S;
 *  (d) NOT PROMISED: the bits of the atomic path, or equality of the single-vector and the block bits.  They agree to rounding.
 * cholamd_device_schur_launches (tests and diagnostics): launches of the Schur condense / expand sweeps on this device object since its creation, out =
 *   { launches of the atomic sweep kernels, deterministic gather launches, deterministic span launches, pack / unpack launches }.
 *
 * Host side (no device): cholamd_plan_schur_condense_host_nrhs / cholamd_plan_schur_expand_host_nrhs walk the SAME cut lists over a host arena whose
 *   eliminated part is factored: the gather has the block kernel's partition (chol_muln_wave / chol_muln_elem), a span is solved by substitution inside its
 *   own lower triangle.  Layout and argument rules as on the device (no overlap checks).  Deterministic, columns independent; not the device's bits.
 * cholamd_plan_schur_det_counts: out = { FORWARD steps, items, sources, entries of L read, BACKWARD steps, items, sources, entries of L read }.
 * cholamd_plan_schur_det_lists: the lists of one direction in the row formats of cholamd_plan_solve_det_lists; the kept lead step has level = -1. */
int cholamd_schur_condense_nrhs(cholamd_device *d, const double *d_arena, int k, const double *d_B, int64_t ldb, double *d_W, int64_t ldw,
                                double *d_G, int64_t ldg, int nrhs, void *stream);
int cholamd_schur_expand_nrhs(cholamd_device *d, const double *d_arena, int k, const double *d_W, int64_t ldw, const double *d_XT, int64_t ldxt,
                              double *d_X, int64_t ldx, int nrhs, void *stream);
int cholamd_schur_condense_nrhs_f32(cholamd_device *d, const float *d_arena32, int k, const double *d_B, int64_t ldb, double *d_W, int64_t ldw,
                                    double *d_G, int64_t ldg, int nrhs, void *stream);
int cholamd_schur_expand_nrhs_f32(cholamd_device *d, const float *d_arena32, int k, const double *d_W, int64_t ldw, const double *d_XT, int64_t ldxt,
                                  double *d_X, int64_t ldx, int nrhs, void *stream);
int cholamd_device_schur_launches(const cholamd_device *d, int64_t out[4]);
int cholamd_plan_schur_condense_host_nrhs(const cholamd_plan *p, int k, const double *arena_host, const double *B, int64_t ldb, double *W, int64_t ldw,
                                          double *G, int64_t ldg, int nrhs);
int cholamd_plan_schur_expand_host_nrhs(const cholamd_plan *p, int k, const double *arena_host, const double *W, int64_t ldw, const double *XT, int64_t ldxt,
                                        double *X, int64_t ldx, int nrhs);
int cholamd_plan_schur_det_counts(const cholamd_plan *p, int k, int64_t out[8]);
int cholamd_plan_schur_det_lists(const cholamd_plan *p, int k, int which, int64_t *steps, int64_t *items, int64_t *srcs);
/* average device time (ms) of the three kernel families of the last cholamd_factor call measured
 * with HIP events on its stream; valid after cholamd_device_sync.  Enable with set_timing(1). */
int cholamd_device_set_timing(cholamd_device *d, int on);
int cholamd_device_get_timing(cholamd_device *d, float ms_by_kind[4], int launches_by_kind[4]);
/* the same with the kinds of a sharded run: [0..3] as above (POTRF (+ fused TRSM), TRSM, update, program launch), [4] the RCCL
 * extend-add exchange, [5] the grouped ncclBroadcasts of the distributed top levels, [6..7] unused */
int cholamd_device_get_timing_ex(cholamd_device *d, float ms_by_kind[8], int launches_by_kind[8]);
/* mean elapsed time (ms) of an event pair with nothing between them on `stream`: the part of every timed launch
 * above that is the event commands, not the kernel */
int cholamd_device_event_overhead(cholamd_device *d, void *stream, float *ms_out);

/* ----------------------------------------------------------------------------------------- */
/* Multi-GPU (not in the reference, whose Legion runtime would move instances          */
/* implicitly): one rank per GPU, the separator tree cut at level log2(world).  Rank g factors    */
/* the subtrees under its level-d separator (cholamd_device_set_partition), its contributions to  */
/* the shared top of the tree accumulate in its own copy of the arena TAIL (the top panels are    */
/* contiguous: offset cholamd_device_tail_offset), ONE RCCL all-reduce (sum, fp64) over that tail  */
/* is the extend-add exchange, then the top levels: REPLICATED on every rank (small roots: they   */
/* are a latency chain) or, option "dist_top" (automatic from a root separator of 1024 columns),  */
/* DISTRIBUTED by column blocks: block b of a top separator belongs to rank (b + heap index) mod  */
/* world; its owner factors it and solves the rows below it, ncclBroadcast carries the block to    */
/* every rank, every rank applies the trailing update and the extend-add to the column blocks IT    */
/* owns (one owner per element, sources in program order: deterministic).  libcholamd links RCCL;   */
/* the communicator is an ncclComm_t made here or adopted from the caller.                         */
/* ----------------------------------------------------------------------------------------- */
typedef struct cholamd_comm cholamd_comm;
#define CHOLAMD_UNIQUE_ID_BYTES 128
int cholamd_comm_unique_id(char id[CHOLAMD_UNIQUE_ID_BYTES]);   /* ncclGetUniqueId: rank 0 calls it and hands the bytes to every rank */
int cholamd_comm_create(cholamd_device *d, int world, int rank, const char id[CHOLAMD_UNIQUE_ID_BYTES], cholamd_comm **out); /* ncclCommInitRank on d's GPU (collective) */
int cholamd_comm_create_all(cholamd_device *const *devs, int n, cholamd_comm **out /* n handles */); /* one process, n GPUs: ncclCommInitAll */
/* one process, n rank objects, NO RCCL: device-side ordered sum of the tails + peer copies, events between the ranks' streams.
 * The ranks may share a device (the one-GPU test box runs world 2 ... 8 this way).  For cholamd_factor_multi only. */
int cholamd_comm_create_local(cholamd_device *const *devs, int n, cholamd_comm **out /* n handles */);
int cholamd_comm_adopt(void *nccl_comm /* ncclComm_t */, int world, int rank, cholamd_comm **out);  /* the caller keeps ownership of the ncclComm_t */
int cholamd_comm_count(const cholamd_comm *c, int *ranks_out); /* ncclCommCount: the ranks the communicator really joins */
void cholamd_comm_destroy(cholamd_comm *c);
int cholamd_comm_allreduce(cholamd_comm *c, double *d_buf, int64_t count, void *stream); /* in-place fp64 sum (ncclAllReduce), asynchronous on `stream` */
/* Per-rank arenas (multi-GPU).  An arena of cholamd_plan_arena_doubles() elements of elem_bytes (8: fp64, 4: the fp32 factor) for this rank: its
 * address range is complete, so every entry point takes it like a plain allocation, but only the rank's own panels (the subtrees cholamd_device_set_partition
 * gave it) and the shared top of the tree are backed by memory of their own (hipMemAddressReserve / hipMemCreate / hipMemMap); the ranges of the other
 * ranks' panels -- never read on this rank -- all alias one 64 MB scratch chunk.  Rank 0 (it gathers the factor and solves) and single-GPU devices get a
 * plain hipMalloc.  Call after cholamd_device_set_partition; *backed_bytes = device memory the arena takes; free with cholamd_device_free_arena (any
 * arena of cholamd_device_alloc / _alloc_arena). */
int cholamd_device_alloc_arena(cholamd_device *d, int elem_bytes, void **dptr, int64_t *backed_bytes);
int cholamd_device_free_arena(cholamd_device *d, void *dptr);
int64_t cholamd_device_tail_offset(const cholamd_device *d);    /* first double of the shared top of the tree in the arena (arena size if world == 1) */
/* the extend-add exchange alone, asynchronous on `stream`.  Replicated top levels: in-place ncclAllReduce(sum) of d_arena[tail .. arena).
 * Top levels distributed by column blocks (option "dist_top"): OWNER-DIRECTED -- a rank works only on the column blocks it owns after the
 * exchange, so every rank sends its partial copy of each block it does not own straight to the owner (grouped ncclSend / ncclRecv:
 * point-to-point over all xGMI links at once) and the owner adds the world - 1 copies to its own in rank order (deterministic).  Each
 * rank receives (world - 1) x its owned blocks and sends the others once: (world - 1) / world of the tail each way, half a ring
 * all-reduce's volume; blocks a rank does not own hold partial sums afterwards and are overwritten by the owners' broadcasts. */
int cholamd_exchange_tail(cholamd_device *d, double *d_arena, cholamd_comm *c, void *stream);
/* elements this rank receives / sends in that exchange, elements of the tail, column-block pieces (0 pieces: the all-reduce) */
int cholamd_exchange_volume(const cholamd_device *d, int64_t out[4]);
/* one rank's part of a sharded factorisation: local levels, exchange, top levels; asynchronous on `stream`.
 * The arena must have been filled by cholamd_device_fill AFTER cholamd_device_set_partition (rank-aware fill).  New values of A
 * (cholamd_device_set_values) belong to a device object: every rank's object needs the call, with the same value array, before its fill. */
int cholamd_factor_sharded(cholamd_device *d, double *d_arena, cholamd_comm *c, void *stream);
/* the same with the fp32 factor (mixed precision x multi-GPU, BASELINE config 5): fp32 arena (cholamd_device_fill_f32 after
 * set_partition), the fp32 schedule partitioned like the fp64 one, exchange and broadcasts on floats */
int cholamd_factor_sharded_f32(cholamd_device *d, float *d_arena32, cholamd_comm *c, void *stream);
/* the panels of the subtrees this rank owns travel to rank 0 (grouped ncclSend / ncclRecv), whose arena then holds the complete
 * factor -- for cholamd_solve / cholamd_solve_refine on rank 0 and the writers.  elem_bytes: 8 (fp64 arena) or 4 (fp32 arena) */
int cholamd_gather_to_root(cholamd_device *d, void *d_arena, int elem_bytes, cholamd_comm *c, void *stream);
/* the same for one process driving n GPUs (devs[g] partitioned as rank g of n): the n all-reduces form one RCCL group */
int cholamd_factor_multi(cholamd_device *const *devs, double *const *arenas, cholamd_comm *const *comms, int n, void *const *streams /* or NULL */);
/* after cholamd_factor_multi: peer-copies the panels of the subtrees owned by ranks 1..n-1 into arenas[0], which then
 * holds the complete factor (for cholamd_solve and the writers) */
int cholamd_gather_factor(cholamd_device *const *devs, double *const *arenas, int n, void *const *streams /* or NULL */);
/* both for the fp32 factor */
int cholamd_factor_multi_f32(cholamd_device *const *devs, float *const *arenas32, cholamd_comm *const *comms, int n, void *const *streams /* or NULL */);
int cholamd_gather_factor_f32(cholamd_device *const *devs, float *const *arenas32, int n, void *const *streams /* or NULL */);
/* Distributed solve (mmat.rg:1394-1479 sharded like the factorisation): every rank sweeps the separators of its own subtrees, the shared top of the
 * tree -- which every rank holds completely after cholamd_factor_sharded / _multi -- is solved redundantly, and only VECTORS travel: one sum over the
 * ranks of the top's part of the right-hand side after the forward sweep under the cut, one sum of the solution at the end (RCCL all-reduces;
 * device-side ordered sums + peer copies over a local communicator).  Every rank passes the same b and ends with the same x.  _f32: an fp32 factor
 * (solution to fp32-factor accuracy); cholamd_solve_refine_sharded: the fp64 iterative refinement of cholamd_solve_refine, every rank running the same
 * loop on identical iterates (residual against A on every rank, corrections solved as above).  No cholamd_gather_to_root is needed for either. */
/* host-side view of rank's share of the solve lists of one tree level: out = { separators, (ancestor, separator) row runs, forward row chunks, backward row
 * chunks, columns solved }; below the cut the ranks' shares tile the undivided lists, above it every rank holds them whole */
int cholamd_plan_solve_counts(const cholamd_plan *p, int level, int rank, int world, int64_t out[5]);
/* what the solve does not read of a level's panels (the structural zeros of the LEAVES: nothing reaches a leaf from below, so its factor stays inside
 * the envelope of A).  seps: 3 ints per separator of the level's list -- first position in the permuted vector, columns, band (L(i, j) = 0 inside the
 * diagonal block for i - j > band; 0: read whole); runs: 5 ints per (ancestor, separator) row run -- first position of the run's rows in the permuted
 * vector, rows, first position of the separator's columns, columns, c_lo (the run's rows are zero in the separator's columns [0, c_lo)).  Counts as in
 * cholamd_plan_solve_counts(p, level, 0, 1, .): out[0] separators, out[1] runs. */
int cholamd_plan_solve_skips(const cholamd_plan *p, int level, int *seps, int *runs);
int cholamd_solve_sharded(cholamd_device *d, const double *d_arena, const double *d_b, double *d_x, cholamd_comm *c, void *stream);
int cholamd_solve_sharded_f32(cholamd_device *d, const float *d_arena32, const double *d_b, double *d_x, cholamd_comm *c, void *stream);
int cholamd_solve_refine_sharded(cholamd_device *d, const float *d_arena32, const double *d_b, double *d_x, int max_iter, double tol,
                                 int *iters_out, double *relres_out, cholamd_comm *c, void *stream);
/* the same driven by one process for n rank objects (communicators of cholamd_comm_create_all or cholamd_comm_create_local); bs[g], xs[g]: rank g's
 * device copies of b and x */
int cholamd_solve_multi(cholamd_device *const *devs, const double *const *arenas, const double *const *bs, double *const *xs, cholamd_comm *const *comms,
                        int n, void *const *streams);
int cholamd_solve_refine_multi(cholamd_device *const *devs, const float *const *arenas32, const double *const *bs, double *const *xs, int max_iter, double tol,
                               int *iters_out, double *relres_out, cholamd_comm *const *comms, int n, void *const *streams);

/* ----------------------------------------------------------------------------------------- */
/* L-B: task level -- the four fused leaf tasks of blas.rg.  A region is a block instance:     */
/* device pointer of element (lo_x, lo_y), leading dimension, and its bounds in permuted         */
/* matrix coordinates (what get_raw_ptr_2d, blas.rg:35-43, resolves from Legion).                */
/* filled lists are HOST arrays, exactly the `Filled` records the reference tasks iterate.       */
/* ----------------------------------------------------------------------------------------- */
typedef struct cholamd_region {
  double *ptr;
  int ld;
  int lo_x, lo_y, hi_x, hi_y;
  const int *tile_row; /* NULL: every row lo_x..hi_x is stored, row x at ptr + (x - lo_x).  Else (row-compacted block instance of the arena):
                        * 16-row tile t of the block (rows lo_x + 16 t ..) is stored at rows 16 * tile_row[t] .. from ptr, or not at all (-1: no
                        * filled tile touches it -- the reference never reads or writes those rows, blas.rg:385-395) */
} cholamd_region;
/* the block instance (r, c) of an arena laid out by `plan` (tile_row points into the plan) */
int cholamd_plan_region(const cholamd_plan *plan, double *d_arena, int r, int c, cholamd_region *out);

/* fused_dpotrf, blas.rg:292-315.  Returns LAPACK info of the first failing tile (the reference discards it). */
int cholamd_fused_dpotrf(const cholamd_region *rA, const cholamd_filled *filled_rA, int nA, int level, int interval, int debug, void *stream);
/* fused_dtrsm, blas.rg:317-351 */
int cholamd_fused_dtrsm(const cholamd_region *rA, const cholamd_region *rB, const cholamd_filled *filled_rA, int nA,
                        const cholamd_filled *filled_rB, int nB, int level, int interval, int debug, void *stream);
/* fused_dsyrk, blas.rg:353-436 */
int cholamd_fused_dsyrk(const cholamd_region *rA, const cholamd_region *rB, const cholamd_region *rC,
                        const cholamd_filled *filled_rA, int nA, const cholamd_filled *filled_rB, int nB,
                        const cholamd_filled *filled_rC, int nC, int col_cluster_size, int level, int interval, int debug, void *stream);
/* fused_dgemm, blas.rg:438-504 */
int cholamd_fused_dgemm(const cholamd_region *rA, const cholamd_region *rB, const cholamd_region *rC,
                        const cholamd_filled *filled_rA, int nA, const cholamd_filled *filled_rB, int nB,
                        const cholamd_filled *filled_rC, int nC, int col_cluster_size, int level, int interval, int debug, void *stream);

/* ----------------------------------------------------------------------------------------- */
/* L-A: BLAS level -- the C symbols Terra binds (blas.rg:71, 99, 139, 187, 226, 263;           */
/* mmat.rg:1057).  Enum values are CBLAS's.  Only the parameter combinations the reference      */
/* issues are implemented; anything else sets cholamd_last_error and returns/raises ERR_ARG.    */
/* `_dev` variants: device pointers, asynchronous on `stream`.                                   */
/* ----------------------------------------------------------------------------------------- */
enum { CholamdColMajor = 102, CholamdNoTrans = 111, CholamdTrans = 112, CholamdUpper = 121, CholamdLower = 122,
       CholamdNonUnit = 131, CholamdLeft = 141, CholamdRight = 142 };

int cholamd_LAPACKE_dpotrf(int matrix_layout, char uplo, int n, double *a, int lda);                      /* blas.rg:71 */
void cholamd_cblas_dtrsm(int layout, int side, int uplo, int transa, int diag, int m, int n, double alpha,
                         const double *a, int lda, double *b, int ldb);                                   /* blas.rg:99 */
void cholamd_cblas_dgemm(int layout, int transa, int transb, int m, int n, int k, double alpha, const double *a, int lda,
                         const double *b, int ldb, double beta, double *c, int ldc);                      /* blas.rg:139 */
void cholamd_cblas_dsyrk(int layout, int uplo, int trans, int n, int k, double alpha, const double *a, int lda,
                         double beta, double *c, int ldc);                                                /* blas.rg:187 */
void cholamd_cblas_dtrsv(int layout, int uplo, int transa, int diag, int n, const double *a, int lda, double *x, int incx); /* blas.rg:226 */
void cholamd_cblas_dgemv(int layout, int trans, int m, int n, double alpha, const double *a, int lda, const double *x, int incx,
                         double beta, double *y, int incy);                                               /* blas.rg:263 */
void cholamd_openblas_set_num_threads(int num_threads);                                                  /* mmat.rg:1057: accepted, no effect */
int cholamd_blas_status(void); /* 0, or the error code of the last L-A call on this thread */

int cholamd_dpotrf_dev(int n, double *d_a, int lda, int *d_info, void *stream);
int cholamd_dtrsm_dev(int m, int n, const double *d_a, int lda, double *d_b, int ldb, void *stream);
int cholamd_dgemm_dev(int m, int n, int k, const double *d_a, int lda, const double *d_b, int ldb, double *d_c, int ldc, void *stream);
int cholamd_dsyrk_dev(int n, int k, const double *d_a, int lda, double *d_c, int ldc, void *stream);
int cholamd_dtrsv_dev(int trans, int n, const double *d_a, int lda, double *d_x, void *stream);
int cholamd_dgemv_dev(int trans, int m, int n, const double *d_a, int lda, const double *d_x, double *d_y, void *stream);

/* ---- low-rank corrections on the finished factor (not in the reference): solves, log det and variances of A + U U^T, A - U U^T and of A under the linear
 * constraints U^T x = e, with U a few dense columns (n x k, column-major, ORIGINAL dof order, 1 <= k <= CHOLAMD_LOWRANK_MAX), without touching the factor's
 * pattern.  CONVENTIONS: M = P^T L P, M M^T = A (the half solves above); Y = M^-1 U; G = Y^T Y = U^T A^-1 U; the CAPACITANCE matrix C = L_C L_C^T (k x k) is
 *     CHOLAMD_LOWRANK_UPDATE     (A + U U^T) x = b                      C = I + G
 *     CHOLAMD_LOWRANK_DOWNDATE   (A - U U^T) x = b, A - U U^T SPD       C = I - G
 *     CHOLAMD_LOWRANK_CONSTRAINT A x + U lambda = b, U^T x = e          C = G
 * V = M^-T Y = A^-1 U, and the object stores W = V L_C^-T (n x k).  Then A'^-1 = A^-1 - sigma W W^T with sigma = -1 for a downdate and +1 otherwise:
 *     corrected solve   x0 = A^-1 b, t = W^T b (constraint mode: t = W^T b - L_C^-1 e), x = x0 - sigma W t
 *     determinant       log det(A +- U U^T) = log det A + log det C, log det C = 2 sum_i log (L_C)_ii        (cholamd_lowrank_logdet)
 *     diagonal          diag(A'^-1) = diag(A^-1) - sigma w, w_i = sum_j W_ij^2: subtract from (add to, for a downdate) cholamd_selinv_diag; in constraint
 *                       mode these are the marginal variances under the constraints                              (cholamd_lowrank_diag)
 *     projection        x* = x - W L_C^-1 (U^T x - e) puts a sample x ~ N(mu, A^-1) on the constraint set         (cholamd_lowrank_project)
 * After cholamd_lowrank_set a corrected solve is one plain solve plus two passes over W (2 n k doubles): no triangular solve with C (its inverse factor
 * R = L_C^-T is kept, k x k) and no pass over L per column of U.
 * cholamd_lowrank_create: an object for up to kmax columns on device object d: ONE n x kmax block, four kmax x kmax / kmax x 32 matrices and the workspace of
 *   the transposed product, all from the device object's allocator (CHOLAMD_POISON and the guard tails apply, cholamd_debug_live_buffers counts them).  The
 *   object refers to d: destroy it first.
 * cholamd_lowrank_set: U is copied into the block; Y by cholamd_solve_half_nrhs(FORWARD) in place; G by the transposed-product kernel; C formed and factored
 *   by cholamd_dpotrf_dev; V by cholamd_solve_half_nrhs(BACKWARD) in place; R = L_C^-T by cholamd_dtrsm_dev on a k x k identity; W = V R in place by the
 *   row-owned product kernel.  The half solves honour the device's solve options: under "solve_deterministic" + "solve_deterministic_block" two calls give
 *   the same bits of W and L_C (everything else in the chain is deterministic whatever the options).  SYNCHRONISES (it returns info).  C not positive
 *   definite -- a downdate too large, dependent or zero constraint columns -- returns CHOLAMD_ERR_ARG, cholamd_last_error names the failing leading minor
 *   (info > 0 in cholamd_lowrank_state) and the object is left UNSET.  k < 1, k > kmax, ldu < n, a NULL pointer, a mode other than the three, a
 *   partitioned device object of rank != 0: CHOLAMD_ERR_ARG, the object keeps the state it had.
 * Any use of an unset object (solve, solve_nrhs, project, diag, logdet, factor, block) returns CHOLAMD_ERR_ARG and writes nothing.
 * cholamd_lowrank_state: out = { k (0: unset), mode, info of the last set }.
 * cholamd_lowrank_solve / _solve_nrhs: the corrected solve, asynchronous on `stream`.  d_e / d_E (k doubles / k x nrhs, lde >= k) are read in constraint mode
 *   only, NULL = zero.  In place (x == b; X == B with ldx == ldb) is allowed: t is taken before the plain solve overwrites b.  The argument rules of
 *   cholamd_solve_nrhs hold verbatim (nrhs == 0 returns 0 and touches nothing; nrhs < 0, ldb < n, ldx < n, a NULL pointer with nrhs > 0: CHOLAMD_ERR_ARG; rows
 *   n .. ld - 1 and columns >= nrhs of X are never written).  Columns go in chunks of 32: per chunk t, then cholamd_solve_nrhs on the chunk (cholamd_solve for
 *   the single vector) with every solve_* option in force, then the correction.  The correction X - X0 of column j depends on column j of B and E alone,
 *   whatever nrhs, the column's chunk and the other columns hold (a NaN there never reaches it), and has the same bits every call.
 * cholamd_lowrank_project: d_xout = d_x - W L_C^-1 (U^T d_x - e) with the caller's U (the object keeps W, not U); constraint mode only; d_e NULL = zero;
 *   d_xout == d_x allowed.  cholamd_lowrank_diag: d_w[i] = sum_j W_ij^2 (n doubles).  cholamd_lowrank_logdet: *logdet_C_out (HOST) = log det C, summed on the
 *   host in index order at set time.  cholamd_lowrank_factor: h_LC (HOST, k x k, ldl >= k) = L_C, the strict upper triangle zero.  cholamd_lowrank_block:
 *   the stored W on the device, read-only, valid until the next set or destroy.
 * DETERMINISM of the kernels (chol_lowrank.hip): T = P^T Q sums the rows in SLABS of 1024 rows -- a partition of n alone, never of k, m or the grid: one
 *   workgroup per slab keeps the slab's partial 16 x 16 tiles (v_mfma_f64_16x16x4_f64) and stores them, a second launch adds an element's partials in slab
 *   order; X = alpha X + beta V T owns rows in chunks of 16; w_i sums j ascending.  One owner per element, no floating-point atomics, no flags, no waits inside
 *   a launch; ragged sizes are masked by selection, never by multiplying with zero.
 * SCOPE: the COMPLETE fp64 factor in the arena: a single-GPU device object, or rank 0's after a gather; another rank: CHOLAMD_ERR_ARG.  There are no _f32 and
 *   no sharded forms.  W belongs to the arena's VALUES at set time: after a refactorisation call cholamd_lowrank_set again -- NOTHING detects a stale W.  One
 *   call at a time per object and per device object.
 * Host restatements (no device) of the kernels' partition: cholamd_lowrank_slabs returns the number of slabs of n rows and writes their first rows
 *   (first_row NULL: the count only; at most cap entries); cholamd_lowrank_tprod_host: T (k x m, ldt >= k) = P^T Q, P n x k, Q n x m, slab by slab;
 *   cholamd_lowrank_rprod_host: X (n x m) = alpha X + beta V T, V n x k, T k x m, in 16-row chunks read whole before they are written (X == V with m == k
 *   allowed; alpha == 0: X is not read).  Leading dimensions at least the row counts (and 1), k <= CHOLAMD_LOWRANK_MAX; k == 0 or m == 0 touches nothing. */
typedef struct cholamd_lowrank cholamd_lowrank;
#define CHOLAMD_LOWRANK_MAX 256
#define CHOLAMD_LOWRANK_UPDATE 1
#define CHOLAMD_LOWRANK_DOWNDATE (-1)
#define CHOLAMD_LOWRANK_CONSTRAINT 0
int  cholamd_lowrank_create(cholamd_device *d, int kmax, cholamd_lowrank **out);
void cholamd_lowrank_destroy(cholamd_lowrank *lr);
int  cholamd_lowrank_set(cholamd_lowrank *lr, const double *d_arena, const double *d_U, int64_t ldu, int k, int mode, void *stream);
int  cholamd_lowrank_state(const cholamd_lowrank *lr, int out[3]);
int  cholamd_lowrank_solve(cholamd_lowrank *lr, const double *d_arena, const double *d_b, const double *d_e, double *d_x, void *stream);
int  cholamd_lowrank_solve_nrhs(cholamd_lowrank *lr, const double *d_arena, const double *d_B, int64_t ldb, const double *d_E, int64_t lde, double *d_X, int64_t ldx, int nrhs, void *stream);
int  cholamd_lowrank_project(cholamd_lowrank *lr, const double *d_U, int64_t ldu, const double *d_x, const double *d_e, double *d_xout, void *stream);
int  cholamd_lowrank_diag(cholamd_lowrank *lr, double *d_w, void *stream);
int  cholamd_lowrank_logdet(cholamd_lowrank *lr, double *logdet_C_out);
int  cholamd_lowrank_factor(cholamd_lowrank *lr, double *h_LC, int ldl);
int  cholamd_lowrank_block(cholamd_lowrank *lr, const double **d_W, int64_t *ldw);
int  cholamd_lowrank_slabs(int64_t n, int64_t *first_row, int64_t cap);
int  cholamd_lowrank_tprod_host(int64_t n, int k, int m, const double *P, int64_t ldp, const double *Q, int64_t ldq, double *T, int64_t ldt);
int  cholamd_lowrank_rprod_host(int64_t n, int k, int m, double alpha, double beta, const double *V, int64_t ldv, const double *T, int64_t ldt, double *X, int64_t ldx);

/* ---- sparse solves: a right-hand side that is non-zero on a few dofs, a solution wanted on a few dofs (CHOLMOD's solve2 with Bset / Xset; DESIGN.md
 * section 19).  L^-1 P b is non-zero only on the separators that hold a non-zero of b and on their ancestors, up(in); x on a dof set needs the backward
 * sweep only on the separators of those dofs and their ancestors, up(out).  The handle owns the step lists of the deterministic block solve PRUNED to these
 * sets (steps, items and sources of the full lists, in their order; per level the descriptors of the active separators), built and uploaded at
 * cholamd_sparse_create: a warm cholamd_sparse_solve_nrhs allocates nothing and only enqueues on `stream`.  The sweeps are the block kernels of option
 * "solve_deterministic_block" on those lists; two small kernels (chol_sparse.hip) load and store the few rows.  NOTHING outside the active rows of the
 * device object's permuted block, and no entry of the arena outside the listed strips and the active separators' diagonal blocks, is read or written.
 * ARGUMENTS: dofs in original order, 0-based.  Bs is n_in x nrhs column-major, ldb >= n_in: row i is the value at in_dofs[i], b is zero everywhere else
 * (an explicit 0.0 is fine; all columns share the pattern).  Xs is n_out x nrhs, ldx >= n_out: row i is x[out_dofs[i]].  which = -1: x = A^-1 b;
 * CHOLAMD_HALF_FORWARD: M^-1 b -- the sweep runs on up(in), an output dof outside it is exactly +0.0; CHOLAMD_HALF_BACKWARD: M^-T b -- the sweep runs on
 * up(out), an input dof outside it cannot reach a wanted output and does not.  The whole solve: up(in), then up(out).  nrhs = 0 returns 0 and touches nothing.
 * REFUSED with CHOLAMD_ERR_ARG, the message naming the first offender, nothing written: a NULL; n_in < 1 or n_out < 1; a dof outside [0, n); a duplicate
 * inside either list; ldb < n_in or ldx < n_out; nrhs < 0; a `which` other than the three; a device object that is another rank of a partition.
 * The handle borrows the device object's permuted block and its workspace of 16x16 inverses: one stream of work per device object covers it.  It forms the
 * inverses of its active separators at every call and does not read or change keep_inverses or any solve_* / schur_* option: it always takes the step
 * kernels.  It needs the COMPLETE factor in the arena, as cholamd_solve_nrhs does, and refers to d: destroy it first.
 * THE CONTRACT:
 *  (a) the same bits from call to call, from one handle to another on the same dof lists, on a device object created under CHOLAMD_POISON=1, and whatever an
 *      earlier call left in the device object's block;
 *  (b) the bits of column j of Xs depend on the arena and on column j of Bs alone;
 *  (c) with in_dofs = out_dofs = 0 .. n - 1 the bits of cholamd_solve_nrhs / cholamd_solve_half_nrhs under "solve_deterministic" + "solve_deterministic_block"
 *      (the pruned lists are then the full ones, element for element);
 *  (d) otherwise it agrees with those to rounding only: dropping sources moves the remaining ones between the four partial sums of a gather;
 *  (e) rows n_in .. ldb - 1 of Bs, rows n_out .. ldx - 1 of Xs and columns >= nrhs are never read or written; Bs is not modified unless Xs aliases it, which
 *      is allowed only with n_in == n_out and ldb == ldx.
 * cholamd_sparse_counts / cholamd_plan_sparse_counts: out[5 d + 0 .. 4] = active separators, steps, items, sources and entries of L read of direction d
 * (counted as cholamd_plan_solve_det_counts counts them), out[10] = active positions of up(in) | up(out), out[11] = the ranges they form.
 * cholamd_plan_sparse_lists: the pruned lists of one direction in the row formats of cholamd_plan_solve_det_lists, sized by the counts.
 * cholamd_plan_sparse_solve_host_nrhs: the same walk on the HOST over a host arena (the gather with the kernel's own partition, a span by substitution:
 * deterministic, not the device's bits); rows of its block outside the active ranges hold NaN, so a read of one shows. */
typedef struct cholamd_sparse cholamd_sparse;
int  cholamd_sparse_create(cholamd_device *d, const int *in_dofs, int n_in, const int *out_dofs, int n_out, cholamd_sparse **out);
void cholamd_sparse_destroy(cholamd_sparse *s);
int  cholamd_sparse_counts(const cholamd_sparse *s, int64_t out[12]);
int  cholamd_sparse_solve_nrhs(cholamd_sparse *s, const double *d_arena, const double *d_Bs, int64_t ldb, double *d_Xs, int64_t ldx, int nrhs, int which, void *stream);
int  cholamd_sparse_solve_nrhs_f32(cholamd_sparse *s, const float *d_arena32, const double *d_Bs, int64_t ldb, double *d_Xs, int64_t ldx, int nrhs, int which, void *stream);
int  cholamd_plan_sparse_solve_host_nrhs(const cholamd_plan *p, const double *arena_host, const int *in_dofs, int n_in, const int *out_dofs, int n_out, int which,
                                         const double *Bs, int64_t ldb, double *Xs, int64_t ldx, int nrhs);
int  cholamd_plan_sparse_counts(const cholamd_plan *p, const int *in_dofs, int n_in, const int *out_dofs, int n_out, int64_t out[12]);
int  cholamd_plan_sparse_lists(const cholamd_plan *p, const int *in_dofs, int n_in, const int *out_dofs, int n_out, int which, int64_t *steps, int64_t *items, int64_t *srcs);

#ifdef __cplusplus
}
#endif
#endif /* CHOLAMD_H */
