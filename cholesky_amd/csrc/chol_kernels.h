/* Launchers of the HIP kernels (internal, C++).  A launcher that works on the factor takes either precision under one name and resolves on the pointer type of
 * the factor: `template <class TL>` where one kernel template serves both (TL = double or float, explicitly instantiated for the two in the defining .hip:
 * the streamed, block and deterministic solves, the factor queries, the products), a pair of overloads where fp64 and fp32 are different kernels
 * (chol_kernels.hip / chol_kernels_f32.hip: scatter, potrf, trsm, trsm_wt, update, update_mt).  Everything else exists for the fp64 factor only. */
#ifndef CHOL_KERNELS_H
#define CHOL_KERNELS_H
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "chol_plan.h"
/* fp64 factor (chol_kernels.hip) */
int chol_launch_scatter(double *arena, const int64_t *dst, const double *val, int64_t nnz, hipStream_t st);
/* new values of A (cholamd_device_set_values): `parts` = CHOL_VALUES_STATUS (the four status words of the value array, which start at
 * { 0, INT64_MAX, 0, INT64_MAX }) | CHOL_VALUES_GATHER (a_val[e] = vals[a_src[e]], csr_val[k] = vals[csr_src[k]]) in one launch */
#define CHOL_VALUES_STATUS 1
#define CHOL_VALUES_GATHER 2
int chol_launch_set_values(const double *vals, int64_t nz, const unsigned char *cls, double *a_val, const int *a_src, int64_t nnz_a,
                           double *csr_val, const int *csr_src, int64_t ncsr, int parts, int64_t *status, hipStream_t st);
int chol_launch_gather(double *out, const double *in, const int *idx, int64_t n, hipStream_t st); /* out[i] = in[idx[i]] */
int chol_launch_potrf(double *base, double *ws, const chol_potrf_desc *descs, int n, int *info, hipStream_t st);
int chol_launch_potrf_big(double *base, double *ws, const chol_potrf_desc *descs, int n, int *info, hipStream_t st);
int chol_launch_potrf_trsm(double *base, double *ws, const chol_potrf_desc *pdescs, int n_potrf, const chol_trsm_desc *tdescs, int n_trsm,
                           const chol_upd_task *tasks, const chol_upd_src *srcs, int n_task,
                           int *info, int *progress, int progress_base, int *done, int done_target, hipStream_t st);
int chol_launch_program(double *base, double *ws, const chol_job *jobs, int njobs, const chol_wait *waits, const chol_potrf_desc *pdescs, const chol_trsm_desc *tdescs,
                        const chol_upd_task *tasks, const chol_upd_src *srcs, const chol_ext *exts, int *ctr, const int *ctr_total, int epoch, int *head, int head_base,
                        int grid, int *info, int *info_next, unsigned long long *trace, hipStream_t st);
int chol_launch_trsm_w(double *base, const double *ws, const chol_trsm_desc *descs, int n, hipStream_t st);
int chol_launch_trsm_wt(double *base, const double *ws, const chol_trsm_desc *descs, int n, hipStream_t st);
int chol_launch_trsm_big(double *base, const double *ws, const chol_trsm_desc *descs, int n, hipStream_t st);
int chol_launch_dinv(const double *L, int n, int ldl, double *W, hipStream_t st);
int chol_launch_trsm(double *base, const double *ws, const chol_trsm_desc *descs, int n, hipStream_t st);
int chol_launch_update(double *base, const chol_upd_task *tasks, const chol_upd_src *srcs, int ntask, hipStream_t st);
int chol_launch_update_mt(double *base, const chol_upd_task *tasks, const chol_upd_src *srcs, int ntask, int64_t arena_elems, hipStream_t st);
/* streamed solve (chol_solve.hip) */
int chol_launch_permute(const double *in, const int *perm, double *out, int n, int inverse, hipStream_t st);
template <class TL> int chol_launch_solve_dinv(const TL *base, const chol_trsv_desc *descs, int n, int max_n, double *W, hipStream_t st);
/* flags / gen: STEP flags of the device object (one int per separator of a top level, zero at allocation) and its launch counter (host) -- the step launches
 * of the wide top separators (k_solve_step); NULL: launch by launch */
template <class TL> int chol_launch_solve_trsv(const TL *base, const chol_trsv_desc *descs, int n, int max_n, int max_under, const double *W, double *y, int backward, int *flags, int *gen, const double *W256, double *xt, hipStream_t st);
/* explicit inverses of the 256-column diagonal spans of a level's separators (levels of at most 8 separators wider than a span): W256[(separator * spans + span) * 65536
 * + column * 256 + row], from the 16x16 inverses W16 of chol_launch_solve_dinv; passed to chol_launch_solve_trsv (with xt: 8 x 256 doubles of scratch) they turn
 * the span solve of the step launches into a matrix-vector product over sixteen workgroups (k_solve_stepw); NULL: k_solve_step */
#define CHOL_STEPW_MAX_SEPS 128 /* most separators of a level that takes the step launches with explicit span inverses: flags = 16 ints, xt = 256 doubles per separator */
template <class TL> int chol_launch_solve_inv256(const TL *base, const chol_trsv_desc *descs, int n, int max_n, const double *W16, double *W256, hipStream_t st);
template <class TL> int chol_launch_solve_offdiag(const TL *base, const chol_gemv_desc *blocks, const int *items, int n_items, double *y, int backward, hipStream_t st);
int chol_launch_trsv_fwd(const double *base, const chol_trsv_desc *descs, int n, double *y, hipStream_t st);
int chol_launch_gemv_fwd(const double *base, const chol_gemv_desc *descs, const int *grp_start, const int *grp_rows, int ngroups, double *y, hipStream_t st);
int chol_launch_bwd(const double *base, const chol_trsv_desc *descs, const chol_gemv_desc *gd, const int *gstart, int n, double *y, hipStream_t st);
/* the fp64 refinement helpers (chol_solve.hip): r = b - A x with the row blocks' sums of r^2 and b^2, x += dx */
int chol_launch_residual(const int64_t *ptr, const int *col, const double *val, const double *b, const double *x, double *r, int n, double *partial, hipStream_t st);
int chol_launch_axpy1(double *x, const double *dx, int n, hipStream_t st);
/* fp32 factor (chol_kernels_f32.hip) */
int chol_launch_scatter(float *arena, const int64_t *dst, const double *val, int64_t nnz, hipStream_t st);
int chol_launch_potrf(float *base, float *ws, const chol_potrf_desc *descs, int n, int *info, hipStream_t st);
int chol_launch_trsm(float *base, const float *ws, const chol_trsm_desc *descs, int n, hipStream_t st); /* (the fp32 schedule's kinds 1 and 4) */
int chol_launch_trsm_wt(float *base, const float *ws, const chol_trsm_desc *descs, int n, hipStream_t st);
int chol_launch_update(float *base, const chol_upd_task *tasks, const chol_upd_src *srcs, int ntask, hipStream_t st);
int chol_launch_update_mt(float *base, const chol_upd_task *tasks, const chol_upd_src *srcs, int ntask, int64_t arena_elems, hipStream_t st);
/* block solve (chol_solve_nrhs.hip): right-hand sides in chunks of CHOL_NRHS_W columns in a permuted block Y (n x CHOL_NRHS_W, row-major); W16 / W256 as for
 * chol_launch_solve_trsv (W256 NULL: the substitution chain of the 16x16 inverses) */
#define CHOL_NRHS_W 32
int chol_nrhs_launch_permute(const double *B, int64_t ldb, const int *perm, double *Y, double *X, int64_t ldx, int n, int c0, int cols, int inverse, hipStream_t st);
template <class TL> int chol_nrhs_launch_trsv(const TL *base, const chol_trsv_desc *descs, int n, int max_n, int max_under, const double *W16, const double *W256, double *Y, int backward, hipStream_t st);
template <class TL> int chol_nrhs_launch_offdiag(const TL *base, const chol_gemv_desc *blocks, const int *items, int n_items, double *Y, int backward, hipStream_t st);
/* R(:, j) = B(:, j) - A X(:, j), j < cols; partial[2 (j * nb + blk) + {0, 1}] = the row block's sum of r^2 / b^2, nb = (n + 255) / 256 */
int chol_nrhs_launch_residual(const int64_t *ptr, const int *col, const double *val, const double *B, int64_t ldb, const double *X, int64_t ldx, double *R, int64_t ldr,
                              int n, int cols, double *partial, hipStream_t st);
int chol_nrhs_launch_axpy(double *X, int64_t ldx, const double *D, int64_t ldd, int n, int cols, hipStream_t st);
/* factor queries (chol_factor_query.hip): one walk over the factor's diagonal for the whole tree.  descs / prefix: the list of chol_diag_list (nd descriptors,
 * prefix[nd] = n).  diag: d_diag[perm[pos]] = L(pos, pos).  logdet: stage 1 writes one partial sum of log L_ii per workgroup (an unevaluated pair hi + lo) to part[2 b], part[2 b + 1] and the workgroup's
 * (entries that are not positive and finite, smallest permuted position of one or INT64_MAX) to ipart[2 b], ipart[2 b + 1]; stage 2 (one workgroup, the
 * partials in a fixed order, as pairs) writes res[0] = the bits of the fp64 sum, res[1] = bad entries, res[2] = the first one's position.  No atomics.
 * part: 2 * CHOL_LOGDET_MAX_BLOCKS doubles, ipart: 2 * CHOL_LOGDET_MAX_BLOCKS int64, res: 3 int64. */
#define CHOL_LOGDET_MAX_BLOCKS 1024
template <class TL> int chol_launch_factor_diag(const TL *base, const chol_trsv_desc *descs, const int *prefix, int nd, int n, const int *perm, double *diag, hipStream_t st);
template <class TL> int chol_launch_factor_logdet(const TL *base, const chol_trsv_desc *descs, const int *prefix, int nd, int n, double *part, int64_t *ipart, int64_t *res, hipStream_t st);
/* selected inversion (chol_selinv.hip): one column-block step of one tree level -- block nblk - 1 - step of the first n_act separators of the level's list
 * (chol_selinv_level, uploaded as it is): L_JJ^-1, Y, the gather-product Z[below, J] and the diagonal block Z[J, J], four launches, no atomics.
 * max_below_tiles: the most 16-row tiles any of them has below the block.  ws: the level's workspace (chol_selinv_level.ws_doubles).
 * entries: vals[k] = quiet NaN for every k < nz, then vals[a_src[e]] = Z[a_dst[e]] for the nnz entries of the scatter list */
int chol_launch_selinv_step(const double *L, double *Z, double *ws, const chol_selinv_sep *seps, int n_act, const chol_selinv_tile *tiles, const int *chain_ld,
                            const int *chain_pos0, const int64_t *rowoff, int step, int max_below_tiles, hipStream_t st);
int chol_launch_selinv_entries(const double *Z, const int64_t *a_dst, const int *a_src, int64_t nnz, double *vals, int64_t nz, hipStream_t st);
/* Schur complement (chol_schur.hip): S (m x m, column-major, leading dimension lds) from the pieces of chol_schur_pieces(p, k, 1, CHOL_SCHUR_CHUNK): both
 * triangles, the zeros of the pieces without storage included; one owner per element, no atomics */
int chol_launch_schur_gather(const double *arena, const chol_schur_desc *descs, int64_t ndesc, double *S, int64_t lds, hipStream_t st);
/* block forms of condense / expand: the transposing copies between the permuted row-major block Y of one chunk (chol_nrhs_launch_permute) and the caller's
 * column-major W (n rows, permuted order), G / XT (m = n - t0 rows, Schur order), columns c0 .. c0 + cols - 1 */
int chol_launch_schur_unpack(const double *Y, int n, int t0, int c0, int cols, double *W, int64_t ldw, double *G, int64_t ldg, hipStream_t st);
int chol_launch_schur_pack(const double *W, int64_t ldw, const double *XT, int64_t ldxt, int n, int t0, int c0, int cols, double *Y, hipStream_t st);
/* forward products with the factor (chol_multiply.hip): one launch over the items of one direction of chol_mul_lists, y = L z (backward = 0) or L^T z (1) in
 * permuted coordinates, z and y distinct; perm != NULL: the result goes to y[perm[pos]] (original dof order).  One owner per element, no atomics.
 * resid: res[0], res[1] = the bits of ||A z - w||^2 and ||A z||^2 (A as CSR in original dof order), res[2] = rows where either is not finite; two stages
 * with one partial pair per workgroup of 256 rows (part: 2 * ceil(n / 256) doubles, ipart: ceil(n / 256) int64), summed in a fixed order */
template <class TL> int chol_launch_multiply(const TL *base, const chol_mul_item *items, int n_items, const chol_mul_src *srcs, int backward, const double *z, double *y, const int *perm, hipStream_t st);
/* deterministic streamed solve (chol_solve_det.hip; chol_plan.h at chol_sdet_lists): the gather launch of one step, y[item] -= sum over the item's sources,
 * `items` = the step's first item, n_items of them, in permuted coordinates and in place (no source of a step is owned by an item of the step); one owner per
 * position, a fixed order, no atomics.  solve_span (chol_solve.hip): the diagonal solve of the columns [col0, col0 + 256) of the n separators `descs`
 * (those with fewer columns do nothing) with the 16x16 inverses W of chol_launch_solve_dinv, plain stores */
template <class TL> int chol_launch_solve_det_gather(const TL *base, const chol_mul_item *items, int n_items, const chol_mul_src *srcs, int backward, double *y, hipStream_t st);
template <class TL> int chol_launch_solve_span(const TL *base, const chol_trsv_desc *descs, int n, const double *W, double *y, int col0, int backward, hipStream_t st);
/* block form of the deterministic solve (option solve_deterministic_block): the gather of one step on a chunk of CHOL_NRHS_W columns,
 * Yp[(item) 32 + j] -= sum over the item's sources, Yp the permuted row-major block of chol_nrhs_launch_permute, in place; the partition of
 * chol_launch_multiply_nrhs (chol_muln_wave / chol_muln_elem), no atomics.  chol_nrhs_launch_span (chol_solve_nrhs.hip): the diagonal solve of the columns
 * [col0, col0 + 256) of the n_descs separators `descs` on the block's 32 columns by the substitution chain of the 16x16 inverses W16 -- that one kernel
 * alone, plain stores */
template <class TL> int chol_launch_solve_det_gather_nrhs(const TL *base, const chol_mul_item *items, int n_items, const chol_mul_src *srcs, int backward, double *Yp, hipStream_t st);
template <class TL> int chol_nrhs_launch_span(const TL *base, const chol_trsv_desc *descs, int n_descs, const double *W16, double *Y, int col0, int backward, hipStream_t st);
/* sparse solves (chol_sparse.hip): a chunk's way into and out of the ACTIVE rows of the permuted row-major block Y.  load: row r of the list, position
 * act_pos[r], takes the chunk's columns of row act_in[r] of Bs (column-major, ldb) or, act_in[r] < 0, zeros; all 32 columns of each of the n_pos rows are
 * written, no other row of Y is touched.  store: Xs[i + (c0 + j) ldx] = Y[pos_out[i] 32 + j], j < cols */
int chol_launch_sparse_load(const double *Bs, int64_t ldb, const int *act_pos, const int *act_in, int64_t n_pos, int c0, int cols, double *Y, hipStream_t st);
int chol_launch_sparse_store(const double *Y, const int *pos_out, int64_t n_out, double *Xs, int64_t ldx, int c0, int cols, hipStream_t st);
/* block form (chol_multiply_nrhs.hip): the same items on a chunk of CHOL_NRHS_W columns, Zp the permuted row-major block of chol_nrhs_launch_permute.
 * perm != NULL (the last stage of a call): Y[perm[pos] + (c0 + j) ldy] for the chunk's columns j < cols; perm == NULL (the first stage of the full product):
 * Y is a second permuted block, all 32 columns written */
template <class TL> int chol_launch_multiply_nrhs(const TL *base, const chol_mul_item *items, int n_items, const chol_mul_src *srcs, int backward, const double *Zp, double *Y, const int *perm,
                                                  int64_t ldy, int c0, int cols, hipStream_t st);
int chol_launch_multiply_resid(const int64_t *ptr, const int *col, const double *val, const double *z, const double *w, int n, double *part, int64_t *ipart, int64_t *res, hipStream_t st);
/* low-rank corrections (chol_lowrank.hip; partition in chol_plan.h at CHOL_LR_SLAB): column-major blocks, k <= CHOL_LR_MAX, no atomics, the same bits every call.
 * tprod: T (k x m) = P^T Q over n rows in two launches per 32 columns of Q (P == Q, ldp == ldq, m == k: the Gram matrix in two launches, lower tiles
 * mirrored); ws: chol_lr_ws_doubles(n, k) doubles.  rprod: X (n x m) = alpha X + beta V T, V n x k, T k x m; X == V with m == k allowed; alpha == 0: X is
 * not read.  rowsq: w[i] = sum_j W(i, j)^2.  small: what = 0: A = I + mode A (mode 0: unchanged), 1: A = I, 2: A -= B, on k x cols */
int64_t chol_lr_ws_doubles(int64_t n, int kmax);
int chol_launch_lr_tprod(int64_t n, int k, int m, const double *P, int64_t ldp, const double *Q, int64_t ldq, double *ws, double *T, int64_t ldt, hipStream_t st);
int chol_launch_lr_rprod(int64_t n, int k, int m, double alpha, double beta, const double *V, int64_t ldv, const double *T, int64_t ldt, double *X, int64_t ldx, hipStream_t st);
int chol_launch_lr_rowsq(int64_t n, int k, const double *W, int64_t ldw, double *w, hipStream_t st);
int chol_launch_lr_small(int what, int k, int cols, int mode, double *A, int64_t lda, const double *B, int64_t ldb, hipStream_t st);
/* gradients with respect to the value array (chol_values_grad.hip): g[k] = alpha s_k + beta g[k] for every k < nz, one owner per entry, no atomics, a fixed
 * order of the sum; beta == 0: g is not read.  pairs: s_k = sum_c (P[i, c] Q[j, c] + P[j, c] Q[i, c]) (one product on the diagonal), (i, j) = (e_row[k],
 * e_col[k]), P and Q column-major in original dof order.  logdet: s_k = m_k Z[a_dst[e]] for the scatter entry e with a_src[e] == k (no two of them share a
 * k: the caller refuses plans with duplicate entries).  Entries with e_cls != CHOL_ENTRY_IN: s_k = 0 */
int chol_launch_values_grad_pairs(const double *P, int64_t ldp, const double *Q, int64_t ldq, int nrhs, const int *e_row, const int *e_col, const unsigned char *e_cls,
                                  int64_t nz, double alpha, double beta, double *g, hipStream_t st);
int chol_launch_values_grad_logdet(const double *Z, const int64_t *a_dst, const int *a_src, int64_t nnz, const int *e_row, const int *e_col, const unsigned char *e_cls,
                                   int64_t nz, double alpha, double beta, double *g, hipStream_t st);
/* preconditioned conjugate gradients and y = A x (chol_pcg.hip): column-major blocks of `cols` <= CHOL_NRHS_W columns, 256 rows per workgroup, no atomics.
 * A partial array holds one double per (column, workgroup) at [j * nb + workgroup], nb = (n + 255) / 256.  rec: one record per column in device memory; the
 * vector kernels read alpha / beta from it (0: the column is not written / p = z), chol_launch_pcg_scalars adds the column's partials in ascending
 * workgroup order and moves the record on by `stage` (INIT, VERIFY and FINAL read the (r^2, b^2) pairs of chol_nrhs_launch_residual).
 *   apply:     Q = A P, partial (may be NULL) = p_i q_i        update: X += alpha P, R -= alpha Q, partial = r_i^2        dot: partial = r_i z_i
 *   direction: P = Z + beta P                                  take:   R = T in the columns of state RESTART */
#define CHOL_PCG_APPLY_G 8 /* columns per lane of the block apply kernel: DESIGN.md section 17 */
enum { CHOL_PCG_CONVERGED = 0, CHOL_PCG_MAXITER = 1, CHOL_PCG_BREAKDOWN = 2, CHOL_PCG_NAN = 3, /* what the caller sees */
       CHOL_PCG_RUNNING = 4, CHOL_PCG_CLAIM = 5 /* rr <= tol^2 bb: the true residual decides */, CHOL_PCG_RESTART = 6 /* runs on from the true residual: p = z */,
       CHOL_PCG_ZERO_B = 7 /* b = 0: x = 0 */ };
enum { CHOL_PCG_STAGE_INIT, CHOL_PCG_STAGE_RHO, CHOL_PCG_STAGE_SIGMA, CHOL_PCG_STAGE_RR, CHOL_PCG_STAGE_VERIFY, CHOL_PCG_STAGE_FINAL };
typedef struct chol_pcg_rec {
  double rho, sigma, alpha, beta, rr, bb, rel; /* r^T z, p^T A p, their quotients, ||r||^2 (recurrence, or true after INIT / VERIFY), ||b||^2, true ||b - A x|| / ||b|| */
  int state, iters, what, pad;                 /* iters: applications of A to p; what: 1 = r^T z, 2 = p^T A p broke down */
} chol_pcg_rec;
int chol_launch_pcg_apply(const int64_t *ptr, const int *col, const double *val, const double *P, int64_t ldp, double *Q, int64_t ldq, int n, int cols, double *partial, hipStream_t st);
int chol_launch_pcg_update(const chol_pcg_rec *rec, const double *P, const double *Q, double *X, int64_t ldx, double *R, int64_t ld, int n, int cols, double *partial, hipStream_t st);
int chol_launch_pcg_dot(const double *R, const double *Z, int64_t ld, int n, int cols, double *partial, hipStream_t st);
int chol_launch_pcg_direction(const chol_pcg_rec *rec, const double *Z, double *P, int64_t ld, int n, int cols, hipStream_t st);
int chol_launch_pcg_take(const chol_pcg_rec *rec, const double *T, double *R, int64_t ld, int n, int cols, hipStream_t st);
int chol_launch_pcg_scalars(chol_pcg_rec *rec, const double *partial, int n, int cols, int stage, double tol, hipStream_t st);
/* diagnostic instance of the program launch (k_program<true>): 4 stamps per job, then CHOL_TRACE_X per job -- [0] follower: own tiles' wait over / update job: wave 0 saw the job's last staged wait hold,
 * [1] its items, [2 + i] round of item i begun; [48 + k] POTRF job: column k published / TRSM job (first strip): column tile k on its channel;
 * [72 + k] POTRF job: the factor wave starts column k / TRSM job: the POTRF's column k seen */
#define CHOL_TRACE_X 96
#endif
