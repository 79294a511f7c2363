// C ABI glue of libcholamd, the solves on a finished factor: the solve lists, the sweep helpers every solve is composed of, the streamed, block, sharded
// and multi-rank solves and the iterative refinements.  Compiled with hipcc like chol_api.cpp; what they share is in chol_device.h.
#include "chol_device.h"

// ---- solve ----------------------------------------------------------------------------------
__global__ void k_zero_ranges(double *y, const int *ranges, int nr)
{ // ranges[2 i], ranges[2 i + 1] = offset, length; one block row per range
  const int off = ranges[2 * blockIdx.y], len = ranges[2 * blockIdx.y + 1];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < len; i += gridDim.x * blockDim.x) y[off + i] = 0.0;
}
// the solve lists of the whole tree (rank 0 of 1: cholamd_solve / cholamd_solve_refine, also on a partitioned device whose arena holds the gathered
// factor) or of one rank's share (the distributed solve); one set is kept, rebuilt when the other is asked for
int build_solve(cholamd_device *d, int rank, int world)
{
  const int L = d->plan->levels;
  if (d->solve_ready && d->solve_rank == rank && d->solve_world == world) return 0;
  free_solve_lists(d);
  d->solve_rank = rank; d->solve_world = world;
  d->sv.resize(L);
  if (world > 1) { // what a rank of the distributed solve starts from zero: every position it does not own, the shared top unless it is rank 0
    const cholamd_plan *p = d->plan;
    std::vector<int> zr;
    for (int s = 1; s <= p->nsep; s++) {
      const int o = chol_owner_of(p, s, world);
      if ((o >= 0 && o != rank) || (o < 0 && rank != 0)) {
        if (!zr.empty() && zr[zr.size() - 2] + zr.back() == p->sep_off[s]) zr.back() += p->sep_size[s];
        else { zr.push_back(p->sep_off[s]); zr.push_back(p->sep_size[s]); }
      }
    }
    d->n_zr_sub = (int)zr.size() / 2;
    { int rc = d->zr_sub.upload(zr.data(), zr.size()); if (rc) return rc; }
  }
  std::vector<chol_trsv_desc> diag; // the whole tree's lists only: the diagonal walk of the factor queries
  for (int lvl = 0; lvl < L; lvl++) {
    chol_solve_level w;
    int rc = chol_build_solve_level_part(d->plan, lvl, rank, world, &w);
    if (rc) return rc;
    if (world == 1) diag.insert(diag.end(), w.trsv, w.trsv + w.n_trsv);
    solve_dev &s = d->sv[lvl];
    s.n_trsv = w.n_trsv; s.n_grp = w.n_grp; s.n_fw = w.n_fw; s.n_bw = w.n_bw;
    rc = s.trsv.upload(w.trsv, (size_t)w.n_trsv);
    if (!rc) rc = s.fw.upload(w.fw, (size_t)w.n_fw);
    if (!rc) rc = s.bw.upload(w.bw, (size_t)w.n_bw);
    if (!rc) rc = s.grp_start.upload(w.grp_start, (size_t)w.n_grp + 1);
    if (!rc) rc = s.grp_rows.upload(w.grp_rows, (size_t)2 * w.n_grp);
    if (!rc) rc = s.bw_start.upload(w.bw_start, (size_t)w.n_trsv + 1);
    s.n_ifw = w.n_ifw; s.n_ibw = w.n_ibw; s.max_n = w.max_n; s.max_under = w.banded && w.max_rows_under_span > 0 ? -w.max_rows_under_span : w.max_rows_under_span;
    if (!rc) rc = s.ifw.upload(w.ifw, (size_t)4 * w.n_ifw);
    if (!rc) rc = s.ibw.upload(w.ibw, (size_t)4 * w.n_ibw);
    chol_solve_level_free(&w);
    if (rc) return rc;
  }
  if (!diag.empty()) {
    std::vector<int> prefix(diag.size() + 1);
    int rc = chol_diag_list(d->plan, diag.data(), (int)diag.size(), prefix.data());
    if (!rc) rc = d->dg_desc.upload(diag.data(), diag.size());
    if (!rc) rc = d->dg_prefix.upload(prefix.data(), prefix.size());
    if (rc) return rc;
    d->n_dg = (int)diag.size();
  }
  int rc = d->ytmp.ensure((size_t)d->plan->n);
  if (!rc) rc = d->ws_solve.ensure((size_t)(d->plan->ws_doubles > 0 ? d->plan->ws_doubles : 1));
  if (!rc) rc = d->step_flags.ensure_zero(CHOL_STEPW_MAX_SEPS * 16);
  if (!rc) rc = d->step_xt.ensure_zero(CHOL_STEPW_MAX_SEPS * 256);
  if (rc) return rc;
  int64_t w256 = 0; // explicit inverses of the diagonal spans where the span chain is the solve's critical path: the levels of at most 8 separators
  if (!std::getenv("CHOLAMD_SOLVE_NO_INV256"))
    for (int lvl = 0; lvl < L; lvl++) {
      solve_dev &s = d->sv[lvl];
      if (s.n_trsv < 1 || s.n_trsv > CHOL_STEPW_MAX_SEPS || s.max_n <= 256 || s.max_under < 0) continue; // (a level of banded leaves: k_solve_leaf32 for an fp32 factor)
      s.w256_off = w256;
      w256 += (int64_t)s.n_trsv * ((s.max_n + 255) / 256) * 65536;
    }
  if (w256 > 0 && (rc = d->w256.alloc((size_t)w256))) return rc;
  d->solve_ready = true;
  return 0;
}

// first position of the shared top of the tree in the permuted vector (the separators above the cut are the last labels: a contiguous tail, as in the arena)
static int64_t top_vec_offset(const cholamd_device *d) { return d->solve_world > 1 ? d->plan->sep_off[d->plan->nsep - (d->solve_world - 1) + 1] : d->plan->n; }
template <class TL> static int lsolve_trsv(cholamd_device *d, const TL *a, const chol_trsv_desc *t, int n, int mx, int mu, const double *W, double *y, int bw, const double *W256, hipStream_t st)
{ return chol_launch_solve_trsv(a, t, n, mx, mu, W, y, bw, d->step_flags, &d->step_gen, W256, d->step_xt, st); } // (the step launches' flags, counter and scratch are the device object's)
// ---- the sweep helpers: every solve, half solve and Schur condense / expand below is a composition of these ----
// The inverses of the diagonal blocks of the levels lvl_lo .. levels - 1 from THIS arena (the factorisation's workspace belongs to the last arena factored): the
// 16x16 ones, and with_spans the explicit span inverses of the wide top separators -- the atomic kernels read them, the deterministic ones do not.  The
// caller decides whether they are due (keep_inverses; once per call in the block forms).
template <class TL> int form_inverses(cholamd_device *d, const TL *d_arena, int lvl_lo, bool with_spans, hipStream_t st)
{
  for (int lvl = lvl_lo; lvl < d->plan->levels; lvl++) {
    const solve_dev &s = d->sv[lvl];
    HIPCHK((hipError_t)chol_launch_solve_dinv(d_arena, s.trsv, s.n_trsv, s.max_n, d->ws_solve, st));
    if (with_spans && s.w256_off >= 0 && d->w256) HIPCHK((hipError_t)chol_launch_solve_inv256(d_arena, s.trsv, s.n_trsv, s.max_n, d->ws_solve, d->w256 + s.w256_off, st));
  }
  return 0;
}
// One sweep of the atomic kernels over the levels lvl_lo .. lvl_hi.  Forward (mmat.rg:1395-1435) from lvl_hi down: TRSV per separator, then its panel into
// the ancestors; backward (mmat.rg:1438-1479) from lvl_lo up: gather from the ancestors, then TRSV^T.  count (the Schur sweeps): 2 more per level.
template <class TL> int sweep_levels(cholamd_device *d, const TL *d_arena, sweep_rhs rhs, bool backward, int lvl_lo, int lvl_hi, int64_t *count, hipStream_t st)
{
  for (int i = 0; i <= lvl_hi - lvl_lo; i++) {
    const solve_dev &s = d->sv[backward ? lvl_lo + i : lvl_hi - i];
    const double *W256 = s.w256_off >= 0 && d->w256 ? d->w256 + s.w256_off : nullptr;
    const int *items = backward ? s.ibw : s.ifw;
    const int n_items = backward ? s.n_ibw : s.n_ifw;
    auto trsv = [&] {
      return rhs.block ? chol_nrhs_launch_trsv(d_arena, s.trsv, s.n_trsv, s.max_n, s.max_under, d->ws_solve, W256, rhs.y, backward, st)
                       : lsolve_trsv(d, d_arena, s.trsv, s.n_trsv, s.max_n, s.max_under, d->ws_solve, rhs.y, backward, W256, st);
    };
    if (!backward) HIPCHK((hipError_t)trsv());
    HIPCHK((hipError_t)(rhs.block ? chol_nrhs_launch_offdiag(d_arena, s.bw, items, n_items, rhs.y, backward, st)
                                  : chol_launch_solve_offdiag(d_arena, s.bw, items, n_items, rhs.y, backward, st)));
    if (backward) HIPCHK((hipError_t)trsv());
    if (count) *count += 2;
  }
  return 0;
}
// One sweep (q: CHOLAMD_HALF_*) of deterministic step lists: per step one gather launch where the step has items and one span launch where it has a span
// (the kept lead step of the cut lists, level -1, is a gather alone).  counts (the Schur sweeps): a gather adds to [1], a span to [2].
template <class TL> int sweep_steps(cholamd_device *d, const TL *d_arena, const sdet_dev &c, int q, sweep_rhs rhs, int64_t *counts, hipStream_t st)
{
  const chol_mul_item *items = c.item[q];
  for (const chol_sdet_step &t : c.step[q]) {
    if (t.item_end > t.item_first) {
      HIPCHK((hipError_t)(rhs.block ? chol_launch_solve_det_gather_nrhs(d_arena, items + t.item_first, t.item_end - t.item_first, c.src[q], q, rhs.y, st)
                                    : chol_launch_solve_det_gather(d_arena, items + t.item_first, t.item_end - t.item_first, c.src[q], q, rhs.y, st)));
      if (counts) counts[1]++;
    }
    if (t.col0 >= 0) {
      const solve_dev &s = d->sv[t.level];
      HIPCHK((hipError_t)(rhs.block ? chol_nrhs_launch_span(d_arena, s.trsv, s.n_trsv, d->ws_solve, rhs.y, t.col0, q, st)
                                    : chol_launch_solve_span(d_arena, s.trsv, s.n_trsv, d->ws_solve, rhs.y, t.col0, q, st)));
      if (counts) counts[2]++;
    }
  }
  return 0;
}
// The streamed solve in three phases, so that a partitioned device can put the two vector reductions of the distributed solve between them:
//   phase 0: y = P b (a rank of a partition: zero outside what it owns), the 16x16 inverses, forward sweep of the levels under the cut
//            -> [sum of the shared top's part of y over the ranks]
//   phase 1: forward and backward sweep of the levels above the cut (every rank: it holds the whole factored top), backward sweep under the cut;
//            ranks other than 0 then clear the top's part again  -> [sum of y over the ranks: every rank has the whole permuted solution]
//   phase 2: x = P^T y
// A device that is not partitioned takes solve_t below, which launches the same with the cut at level 0 and nothing between the phases.
template <class TL> static int solve_phase(cholamd_device *d, const TL *d_arena, const double *d_b, double *d_x, int phase, hipStream_t st)
{
  const int L = d->plan->levels, n = d->plan->n, cut = d->solve_world > 1 ? chol_split_level(d->solve_world) : 0;
  double *y = d->ytmp;
  const sweep_rhs rhs = { y, false };
  int rc = 0;
  if (phase == 0) {
    HIPCHK((hipError_t)chol_launch_permute(d_b, d->perm, y, n, 0, st));
    if (d->n_zr_sub > 0) { hipLaunchKernelGGL(k_zero_ranges, dim3(16, d->n_zr_sub), dim3(256), 0, st, y, d->zr_sub, d->n_zr_sub); HIPCHK(hipGetLastError()); }
    if (!d->keep_inverses && (rc = form_inverses(d, d_arena, 0, true, st))) return rc;
    if ((rc = sweep_levels(d, d_arena, rhs, false, cut, L - 1, nullptr, st))) return rc;
  }
  if (phase == 1) {
    if ((rc = sweep_levels(d, d_arena, rhs, false, 0, cut - 1, nullptr, st))) return rc;
    if ((rc = sweep_levels(d, d_arena, rhs, true, 0, L - 1, nullptr, st))) return rc;
    if (d->solve_world > 1 && d->solve_rank != 0) { // the top's part of the solution is counted once in the sum that follows: rank 0's
      const int64_t t0 = top_vec_offset(d);
      HIPCHK(hipMemsetAsync(y + t0, 0, (size_t)(n - t0) * sizeof(double), st));
    }
  }
  if (phase == 2) HIPCHK((hipError_t)chol_launch_permute(y, d->perm, d_x, n, 1, st));
  return 0;
}
// ---------------------------------------------------------------------------------------------
// The deterministic sweeps (option solve_deterministic; include/cholamd.h at "deterministic solve"): the step lists of chol_sdet_lists walked by sweep_steps
// in place of the atomic kernels.  They need the solve lists of the whole tree (the spans' TRSV descriptors per level) and the 16x16 inverses alone.
// ---------------------------------------------------------------------------------------------
int upload_sdet(sdet_dev &q, const chol_sdet_lists &w)
{
  int rc = 0;
  for (int c = 0; c < 2 && !rc; c++) { // (an upload replaces what a call that failed half-way left)
    rc = q.item[c].upload(w.item[c], (size_t)w.n_item[c]);
    if (!rc) rc = q.src[c].upload(w.src[c], (size_t)w.n_src[c]);
    q.step[c].assign(w.step[c], w.step[c] + w.n_step[c]);
  }
  q.ready = !rc;
  return rc;
}
static int build_solve_det(cholamd_device *d)
{
  if (d->sdet.ready) return 0;
  chol_sdet_lists w;
  int rc = chol_build_solve_det(d->plan, &w);
  if (rc) return rc;
  rc = upload_sdet(d->sdet, w);
  chol_sdet_lists_free(&w);
  return rc;
}
// the sweeps `which` of the whole tree on rhs: the step lists (det) or the atomic kernels level by level
template <class TL> static int sweep_tree(cholamd_device *d, const TL *d_arena, sweep_rhs rhs, int which, bool det, hipStream_t st)
{
  for (int q = 0; q < 2; q++) {
    if (which != CHOL_BOTH_SWEEPS && which != q) continue;
    int rc = det ? sweep_steps(d, d_arena, d->sdet, q, rhs, nullptr, st) : sweep_levels(d, d_arena, rhs, q == CHOLAMD_HALF_BACKWARD, 0, d->plan->levels - 1, nullptr, st);
    if (rc) return rc;
  }
  return 0;
}
// The streamed solve of one vector on the whole tree (every panel read once; a factor of element type TL, vectors and arithmetic fp64): the arena holds the
// complete factor (single GPU, or gathered on this rank).  x = A^-1 b (CHOL_BOTH_SWEEPS), P^T L^-1 P b (CHOLAMD_HALF_FORWARD) or P^T L^-T P b
// (CHOLAMD_HALF_BACKWARD): the permute, the diagonal inverses of THIS arena unless the caller keeps them, the sweeps -- deterministic under option
// solve_deterministic -- and the permute back: what solve_phase launches on a device that is not partitioned.
template <class TL> static int solve_t(cholamd_device *d, const TL *d_arena, const double *d_b, double *d_x, int which, hipStream_t st)
{
  const bool det = d->solve_deterministic;
  { int rc = build_solve(d); if (!rc && det) rc = build_solve_det(d); if (rc) return rc; }
  const int n = d->plan->n;
  double *y = d->ytmp;
  HIPCHK((hipError_t)chol_launch_permute(d_b, d->perm, y, n, 0, st));
  if (!d->keep_inverses) { int rc = form_inverses(d, d_arena, 0, !det, st); if (rc) return rc; }
  { int rc = sweep_tree(d, d_arena, { y, false }, which, det, st); if (rc) return rc; }
  HIPCHK((hipError_t)chol_launch_permute(y, d->perm, d_x, n, 1, st));
  return 0;
}
// the same with the per-call kernels the BLAS-level entry points use (option solve_reference_shape: deterministic, slow at scale; fp64 factor only)
static int solve_reference(cholamd_device *d, const double *d_arena, const double *d_b, double *d_x, int which, hipStream_t st)
{
  { int rc = build_solve(d); if (rc) return rc; }
  const int L = d->plan->levels, n = d->plan->n;
  double *y = d->ytmp;
  HIPCHK((hipError_t)chol_launch_permute(d_b, d->perm, y, n, 0, st));
  for (int lvl = L - 1; lvl >= 0 && which != CHOLAMD_HALF_BACKWARD; lvl--) { // forward, mmat.rg:1395-1435
    const solve_dev &s = d->sv[lvl];
    HIPCHK((hipError_t)chol_launch_trsv_fwd(d_arena, s.trsv, s.n_trsv, y, st));
    HIPCHK((hipError_t)chol_launch_gemv_fwd(d_arena, s.fw, s.grp_start, s.grp_rows, s.n_grp, y, st));
  }
  for (int lvl = 0; lvl < L && which != CHOLAMD_HALF_FORWARD; lvl++) { // backward, mmat.rg:1438-1479
    const solve_dev &s = d->sv[lvl];
    HIPCHK((hipError_t)chol_launch_bwd(d_arena, s.trsv, s.bw, s.bw_start, s.n_trsv, y, st));
  }
  HIPCHK((hipError_t)chol_launch_permute(y, d->perm, d_x, n, 1, st));
  return 0;
}
// One vector by the options in force, first match:
//   solve_reference_shape, fp64 factor -> solve_reference (for an fp32 factor the option has no effect)
//   solve_deterministic                -> solve_t with the step lists
//   otherwise                          -> solve_t with the atomic kernels
template <class TL> int solve_any(cholamd_device *d, const TL *d_arena, const double *d_b, double *d_x, int which, hipStream_t st)
{
  if constexpr (std::is_same<TL, double>::value) { if (d->solve_reference_shape) return solve_reference(d, d_arena, d_b, d_x, which, st); }
  return solve_t(d, d_arena, d_b, d_x, which, st);
}
int half_which_ok(int which, const char *what)
{
  if (which == CHOLAMD_HALF_FORWARD || which == CHOLAMD_HALF_BACKWARD) return 0;
  chol_set_error("%s: which = %d is neither CHOLAMD_HALF_FORWARD (0) nor CHOLAMD_HALF_BACKWARD (1)", what, which);
  return CHOLAMD_ERR_ARG;
}
// cholamd_solve[_f32] (half = false: no argument checks, as ever) and cholamd_solve_half[_f32] (include/cholamd.h at cholamd_solve_half: M = P^T L P, so
// M M^T = A in original dof order): the checks, the device, then solve_any's cascade
template <class TL> static int solve_api(cholamd_device *d, const TL *d_arena, const double *d_b, double *d_x, bool half, int which, hipStream_t st, const char *what)
{
  if (half) {
    if (!d) { chol_set_error("%s: NULL device", what); return CHOLAMD_ERR_ARG; }
    { int rc = half_which_ok(which, what); if (rc) return rc; }
    if (!d_arena || !d_b || !d_x) { chol_set_error("%s: NULL %s", what, !d_arena ? "arena" : !d_b ? "b" : "x"); return CHOLAMD_ERR_ARG; }
  } else which = CHOL_BOTH_SWEEPS;
  HIPCHK(hipSetDevice(d->dev));
  return solve_any(d, d_arena, d_b, d_x, which, st);
}
extern "C" int cholamd_solve(cholamd_device *d, const double *d_arena, const double *d_b, double *d_x, void *stream)
{ return solve_api(d, d_arena, d_b, d_x, false, 0, (hipStream_t)stream, "cholamd_solve"); }
extern "C" int cholamd_solve_f32(cholamd_device *d, const float *d_arena32, const double *d_b, double *d_x, void *stream)
{ return solve_api(d, d_arena32, d_b, d_x, false, 0, (hipStream_t)stream, "cholamd_solve_f32"); }
extern "C" int cholamd_solve_half(cholamd_device *d, const double *d_arena, const double *d_b, double *d_x, int which, void *stream)
{ return solve_api(d, d_arena, d_b, d_x, true, which, (hipStream_t)stream, "cholamd_solve_half"); }
extern "C" int cholamd_solve_half_f32(cholamd_device *d, const float *d_arena32, const double *d_b, double *d_x, int which, void *stream)
{ return solve_api(d, d_arena32, d_b, d_x, true, which, (hipStream_t)stream, "cholamd_solve_half_f32"); }

// r = b - A x on the device (fp64, A = the matrix file's entries, both triangles), ||r|| / ||b|| back on the host
static int residual_norm(cholamd_device *d, const double *d_b, const double *d_x, double *d_r, double *relres, hipStream_t st)
{
  const int n = d->plan->n, nb = (n + 255) / 256;
  HIPCHK((hipError_t)chol_launch_residual(d->csr_ptr, d->csr_col, d->csr_val, d_b, d_x, d_r, n, d->partial, st));
  std::vector<double> h((size_t)2 * nb);
  HIPCHK(hipMemcpyAsync(h.data(), d->partial, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  double r2 = 0.0, b2 = 0.0;
  for (int i = 0; i < nb; i++) { r2 += h[2 * i]; b2 += h[2 * i + 1]; }
  *relres = b2 > 0.0 ? std::sqrt(r2 / b2) : std::sqrt(r2);
  return 0;
}
extern "C" int cholamd_residual(cholamd_device *d, const double *d_b, const double *d_x, double *d_r, double *relres_out, void *stream)
{
  HIPCHK(hipSetDevice(d->dev));
  int rc = ensure_refine(d);
  if (rc) return rc;
  return residual_norm(d, d_b, d_x, d_r, relres_out, (hipStream_t)stream);
}
hipStream_t stream_of(void *const *streams, int g) { return streams ? (hipStream_t)streams[g] : nullptr; }
static int refine_nan_error() { chol_set_error("iterative refinement produced NaN (fp32 factorisation broke down)"); return CHOLAMD_ERR_ARG; }
// The refinement of one vector, written once over n rank objects (1: the single and the sharded form; every rank holds the same b and the same iterate):
// x0 = M^-1 b with M = L32 L32^T; then x += M^-1 (b - A x) until ||b - A x|| <= tol ||b||.  solve(rhs, out) applies M^-1 on every rank.  The callers
// have made their checks and pass the ranks' residual and correction vectors (rv[g] = devs[g]->rvec, dx[g] = devs[g]->dxvec) as the arrays solve takes.
template <class Solve> static int refine_loop(cholamd_device *const *devs, int n, const double *const *bs, double *const *xs, const double *const *rv, double *const *dx,
                                              void *const *streams, int max_iter, double tol, int *iters_out, double *relres_out, Solve solve)
{
  if (max_iter < 0) max_iter = 0;
  int rc = solve(bs, xs);
  if (rc) return rc;
  keep_inverses_scope keep(devs, n);
  double rel = 0.0;
  int it = 0;
  for (;; ++it) {
    for (int g = 0; g < n; g++) { // every rank forms the residual of its own (identical) iterate
      double rg = 0.0;
      HIPCHK(hipSetDevice(devs[g]->dev));
      if ((rc = residual_norm(devs[g], bs[g], xs[g], devs[g]->rvec, &rg, stream_of(streams, g)))) return rc;
      if (g == 0) rel = rg;
    }
    if (!(rel > tol) || it >= max_iter) break; // also leaves on NaN (the same decision on every rank: the iterates are identical)
    if ((rc = solve(rv, dx))) return rc;
    for (int g = 0; g < n; g++) { HIPCHK(hipSetDevice(devs[g]->dev)); HIPCHK((hipError_t)chol_launch_axpy1(xs[g], devs[g]->dxvec, devs[g]->plan->n, stream_of(streams, g))); }
  }
  if (iters_out) *iters_out = it;
  if (relres_out) *relres_out = rel;
  return rel != rel ? refine_nan_error() : 0;
}
extern "C" int cholamd_solve_refine(cholamd_device *d, const float *d_arena32, const double *d_b, double *d_x, int max_iter, double tol,
                                    int *iters_out, double *relres_out, void *stream)
{
  HIPCHK(hipSetDevice(d->dev));
  int rc = ensure_refine(d);
  if (!rc) rc = build_solve(d);
  if (rc) return rc;
  const double *rv = d->rvec;
  double *dx = d->dxvec;
  return refine_loop(&d, 1, &d_b, &d_x, &rv, &dx, &stream, max_iter, tol, iters_out, relres_out,
                     [&](const double *const *r, double *const *o) { return solve_t(d, d_arena32, r[0], o[0], CHOL_BOTH_SWEEPS, (hipStream_t)stream); });
}

// ---------------------------------------------------------------------------------------------
// Block solve (not in the reference, whose mmat.rg -b solves one vector): nrhs right-hand sides in chunks of CHOL_NRHS_W columns, each chunk one forward
// and one backward sweep over the solve lists of the whole tree (chol_solve_nrhs.hip), so the factor is read once per sweep per chunk.
// ---------------------------------------------------------------------------------------------
// in / out: what the entry point's header calls its two blocks (the solves: B, X; the products: Z, Y)
// The argument rules of every block call.  1: nothing to do.  with_arena = false is for the calls that take none (cholamd_apply_nrhs).
int block_check(cholamd_device *d, bool with_arena, const void *arena, const double *B, int64_t ldb, const double *X, int64_t ldx, int nrhs, const char *what, const char *in,
                       const char *out)
{
  if (!d) { chol_set_error("%s: NULL device", what); return CHOLAMD_ERR_ARG; }
  const int n = d->plan->n;
  if (nrhs < 0) { chol_set_error("%s: nrhs = %d < 0", what, nrhs); return CHOLAMD_ERR_ARG; }
  if (ldb < n || ldx < n) {
    std::string li(in), lo(out); // "B" -> ldb, "Z" -> ldz
    for (auto &c : li) c = (char)std::tolower((unsigned char)c);
    for (auto &c : lo) c = (char)std::tolower((unsigned char)c);
    chol_set_error("%s: leading dimensions ld%s = %lld, ld%s = %lld must be at least n = %d", what, li.c_str(), (long long)ldb, lo.c_str(), (long long)ldx, n);
    return CHOLAMD_ERR_ARG;
  }
  if (nrhs == 0) return 1;
  const bool no_arena = with_arena && !arena;
  if (no_arena || !B || !X) { chol_set_error("%s: NULL %s", what, no_arena ? "arena" : !B ? in : out); return CHOLAMD_ERR_ARG; }
  return 0;
}
int nrhs_check(cholamd_device *d, const void *arena, const double *B, int64_t ldb, const double *X, int64_t ldx, int nrhs, const char *what, const char *in, const char *out)
{
  return block_check(d, true, arena, B, ldb, X, ldx, nrhs, what, in, out);
}
// A chunk's sweeps cost the same for 1 and for 32 columns (the launches of the span chain and the factor's bytes, not the MFMA work, set their time), so a
// chunk of fewer columns than this is solved column by column with the single-vector path.  Measured on one MI355X: a block chunk
// takes 3.0 - 3.3 single fp64 solves and 5.0 single fp32-factor solves.
template <class TL> static constexpr int nrhs_min_block() { return sizeof(TL) == sizeof(double) ? 4 : 6; }
// The block body: the diagonal inverses once per call (a caller that keeps them: not at all), then chunk by chunk the permute into the row-major block, the
// sweeps `which` of the whole tree with the chol_nrhs_* kernels, and the permute back.
//   det = false: the atomic kernels; a chunk under the threshold goes column by column through solve_t, which reuses the call's inverses
//   det = true (option solve_deterministic_block; include/cholamd.h at "deterministic solve"): the step lists of solve_t's deterministic sweeps, one block gather
//     (k_solve_det_gather_nrhs) and one k_nrhs_span launch in its substitution form per step; the atomic kernels (k_nrhs_panel, k_nrhs_offdiag) are never
//     launched.  EVERY chunk takes these kernels, whatever its column count: a column's bits must not depend on how many columns travel with it.
template <class TL> static int solve_nrhs_t(cholamd_device *d, const TL *d_arena, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, int which, bool det, hipStream_t st)
{
  { int rc = build_solve(d); if (!rc && det) rc = build_solve_det(d); if (rc) return rc; }
  const int n = d->plan->n, min_block = det ? 1 : which == CHOL_BOTH_SWEEPS ? nrhs_min_block<TL>() : half_nrhs_min_block<TL>();
  if (!d->keep_inverses) { int rc = form_inverses(d, d_arena, 0, !det, st); if (rc) return rc; }
  keep_restore kr(d);
  if (!det) d->keep_inverses = true; // (read by the column-by-column chunks alone)
  for (int c0 = 0; c0 < nrhs; c0 += CHOL_NRHS_W) {
    const int cols = std::min(CHOL_NRHS_W, nrhs - c0);
    if (cols < min_block) {
      for (int j = c0; j < c0 + cols; j++) { int rc = solve_t(d, d_arena, d_B + (int64_t)j * ldb, d_X + (int64_t)j * ldx, which, st); if (rc) return rc; }
      continue;
    }
    { int rc = d->ynrhs.ensure((size_t)n * CHOL_NRHS_W); if (rc) return rc; }
    double *Y = d->ynrhs;
    HIPCHK((hipError_t)chol_nrhs_launch_permute(d_B, ldb, d->perm, Y, nullptr, 0, n, c0, cols, 0, st));
    { int rc = sweep_tree(d, d_arena, { Y, true }, which, det, st); if (rc) return rc; }
    HIPCHK((hipError_t)chol_nrhs_launch_permute(nullptr, 0, d->perm, Y, d_X, ldx, n, c0, cols, 1, st));
  }
  return 0;
}
static bool det_block(const cholamd_device *d) { return d->solve_deterministic && d->solve_deterministic_block && !d->solve_reference_shape; }
// `cols` columns by the options in force (half: one of the half solves), first match:
//   solve_deterministic and solve_deterministic_block, no solve_reference_shape -> solve_nrhs_t, det
//   solve_reference_shape (fp64 factor) or solve_deterministic                  -> column by column through solve_any: both are deterministic there
//   solve_reference_shape, fp32 factor, the full solve                          -> column by column through solve_any: the atomic solve_t (no per-call kernels)
//   otherwise (also: solve_reference_shape, fp32 factor, a half solve)          -> solve_nrhs_t, atomic
template <class TL> int solve_nrhs_any(cholamd_device *d, const TL *d_arena, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int cols, bool half, int which, hipStream_t st)
{
  if (det_block(d)) return solve_nrhs_t(d, d_arena, d_B, ldb, d_X, ldx, cols, which, true, st);
  if (d->solve_deterministic || (d->solve_reference_shape && (!half || std::is_same<TL, double>::value))) {
    for (int j = 0; j < cols; j++) { int rc = solve_any(d, d_arena, d_B + (int64_t)j * ldb, d_X + (int64_t)j * ldx, which, st); if (rc) return rc; }
    return 0;
  }
  return solve_nrhs_t(d, d_arena, d_B, ldb, d_X, ldx, cols, which, false, st);
}
// cholamd_solve_nrhs[_f32] and cholamd_solve_half_nrhs[_f32]: the checks (which before nrhs), the device, then solve_nrhs_any's cascade
template <class TL> static int solve_nrhs_api(cholamd_device *d, const TL *d_arena, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, bool half, int which, hipStream_t st, const char *what)
{
  if (half && d) { int rc = half_which_ok(which, what); if (rc) return rc; }
  if (!half) which = CHOL_BOTH_SWEEPS;
  { int rc = nrhs_check(d, d_arena, d_B, ldb, d_X, ldx, nrhs, what); if (rc) return rc > 0 ? 0 : rc; }
  HIPCHK(hipSetDevice(d->dev));
  return solve_nrhs_any(d, d_arena, d_B, ldb, d_X, ldx, nrhs, half, which, st);
}
extern "C" int cholamd_solve_nrhs(cholamd_device *d, const double *d_arena, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, void *stream)
{ return solve_nrhs_api(d, d_arena, d_B, ldb, d_X, ldx, nrhs, false, 0, (hipStream_t)stream, "cholamd_solve_nrhs"); }
extern "C" int cholamd_solve_nrhs_f32(cholamd_device *d, const float *d_arena32, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, void *stream)
{ return solve_nrhs_api(d, d_arena32, d_B, ldb, d_X, ldx, nrhs, false, 0, (hipStream_t)stream, "cholamd_solve_nrhs_f32"); }
extern "C" int cholamd_solve_half_nrhs(cholamd_device *d, const double *d_arena, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, int which, void *stream)
{ return solve_nrhs_api(d, d_arena, d_B, ldb, d_X, ldx, nrhs, true, which, (hipStream_t)stream, "cholamd_solve_half_nrhs"); }
extern "C" int cholamd_solve_half_nrhs_f32(cholamd_device *d, const float *d_arena32, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, int which, void *stream)
{ return solve_nrhs_api(d, d_arena32, d_B, ldb, d_X, ldx, nrhs, true, which, (hipStream_t)stream, "cholamd_solve_half_nrhs_f32"); }

// one chunk's residuals: R = B - A X (column-major, ld n), rel[j] = ||r_j|| / ||b_j||
static int residual_nrhs(cholamd_device *d, const double *d_B, int64_t ldb, const double *d_X, int64_t ldx, int cols, double *rel, hipStream_t st)
{
  const int n = d->plan->n, nb = (n + 255) / 256;
  HIPCHK((hipError_t)chol_nrhs_launch_residual(d->csr_ptr, d->csr_col, d->csr_val, d_B, ldb, d_X, ldx, d->rnrhs, n, n, cols, d->pnrhs, st));
  std::vector<double> h((size_t)2 * nb * cols);
  HIPCHK(hipMemcpyAsync(h.data(), d->pnrhs, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int j = 0; j < cols; j++) {
    double r2 = 0.0, b2 = 0.0;
    for (int i = 0; i < nb; i++) { r2 += h[2 * ((size_t)j * nb + i)]; b2 += h[2 * ((size_t)j * nb + i) + 1]; }
    rel[j] = b2 > 0.0 ? std::sqrt(r2 / b2) : std::sqrt(r2);
  }
  return 0;
}
// M^-1 B for `cols` columns with M = L32 L32^T: what cholamd_solve_nrhs_f32 runs under the options in force
static int refine_solve(cholamd_device *d, const float *d_arena32, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int cols, hipStream_t st)
{ return solve_nrhs_any(d, d_arena32, d_B, ldb, d_X, ldx, cols, false, CHOL_BOTH_SWEEPS, st); }
extern "C" int cholamd_solve_refine_nrhs(cholamd_device *d, const float *d_arena32, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, int max_iter,
                                         double tol, int *iters_out, double *relres_out, void *stream)
{
  { int rc = nrhs_check(d, d_arena32, d_B, ldb, d_X, ldx, nrhs, "cholamd_solve_refine_nrhs"); if (rc) { if (rc > 0 && iters_out) *iters_out = 0; return rc > 0 ? 0 : rc; } }
  HIPCHK(hipSetDevice(d->dev));
  int rc = ensure_refine(d);
  if (!rc) rc = build_solve(d);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int n = d->plan->n, nb = (n + 255) / 256;
  if (!rc) rc = d->bnrhs.ensure((size_t)n * CHOL_NRHS_W);
  if (!rc) rc = d->rnrhs.ensure((size_t)n * CHOL_NRHS_W);
  if (!rc) rc = d->dxnrhs.ensure((size_t)n * CHOL_NRHS_W);
  if (!rc) rc = d->pnrhs.ensure((size_t)2 * nb * CHOL_NRHS_W);
  if (rc) return rc;
  if (max_iter < 0) max_iter = 0;
  // chunk by chunk: the chunk's columns of B are copied first (X may be B: in place), x0 = M^-1 b with M = L32 L32^T, then X += M^-1 (B - A X) on ALL the
  // chunk's columns until every one of them has ||b_j - A x_j|| <= tol ||b_j|| or max_iter corrections have been applied.  The inverses are formed once.
  keep_inverses_scope keep(&d, 1);
  d->keep_inverses = false; // (until the first solve has formed them)
  int it_max = 0;
  bool nan = false;
  std::vector<double> rel(CHOL_NRHS_W);
  int c0 = 0;
  for (; c0 < nrhs; c0 += CHOL_NRHS_W) {
    const int cols = std::min(CHOL_NRHS_W, nrhs - c0);
    double *X = d_X + (int64_t)c0 * ldx;
    HIPCHK(hipMemcpy2DAsync(d->bnrhs, (size_t)n * sizeof(double), d_B + (int64_t)c0 * ldb, (size_t)ldb * sizeof(double), (size_t)n * sizeof(double), (size_t)cols,
                            hipMemcpyDeviceToDevice, st));
    if ((rc = refine_solve(d, d_arena32, d->bnrhs, n, X, ldx, cols, st))) return rc;
    d->keep_inverses = true;
    int it = 0;
    for (;; ++it) {
      if ((rc = residual_nrhs(d, d->bnrhs, n, X, ldx, cols, rel.data(), st))) return rc;
      bool done = true;
      for (int j = 0; j < cols; j++) { if (rel[j] != rel[j]) nan = true; if (rel[j] > tol) done = false; }
      if (done || nan || it >= max_iter) break;
      if ((rc = refine_solve(d, d_arena32, d->rnrhs, n, d->dxnrhs, n, cols, st))) return rc;
      HIPCHK((hipError_t)chol_nrhs_launch_axpy(X, ldx, d->dxnrhs, n, n, cols, st));
    }
    if (it > it_max) it_max = it;
    if (relres_out) for (int j = 0; j < cols; j++) relres_out[c0 + j] = rel[j];
    if (nan) { c0 += cols; break; }
  }
  if (relres_out) for (int j = c0; j < nrhs; j++) relres_out[j] = std::nan(""); // (after a NaN: the chunks not reached)
  if (iters_out) *iters_out = it_max;
  return nan ? refine_nan_error() : 0;
}

// ---------------------------------------------------------------------------------------------
// Distributed solve (mmat.rg:1394-1479 sharded like the factorisation).  After cholamd_factor_sharded / _multi a rank's arena holds
// the panels of its own subtrees and the WHOLE factored top (replicated, or broadcast block by block under dist_top).  So: every rank sweeps its own
// subtrees forward (the contributions to the top accumulate in its copy of the top's part of y, which starts from b on rank 0 and from zero
// elsewhere), ONE sum of that part over the ranks, every rank solves the top forward and backward redundantly, sweeps its subtrees backward, and one
// sum of the permuted vector (every position is non-zero on exactly one rank) gives every rank the solution.  Only vectors travel: (world - 1) top
// separators' worth of doubles, then n doubles -- against the 17-33 GB of factor that cholamd_gather_to_root moved at 100^3.  The iterative
// refinement runs the same loop on every rank (residual in fp64 against A, replicated; the corrections solved as above): identical iterates.
// ---------------------------------------------------------------------------------------------
template <class TL> static int solve_sharded_t(cholamd_device *d, const TL *d_arena, const double *d_b, double *d_x, cholamd_comm *c, hipStream_t st)
{
  HIPCHK(hipSetDevice(d->dev));
  if (d->world == 1) return solve_t(d, d_arena, d_b, d_x, CHOL_BOTH_SWEEPS, st);
  int rc = build_solve(d, d->rank, d->world);
  if (rc) return rc;
  if (comm_matches(d, c)) return CHOLAMD_ERR_ARG;
  if (!c->comm) { chol_set_error("a local communicator solves through cholamd_solve_multi only"); return CHOLAMD_ERR_ARG; }
  const int64_t t0 = top_vec_offset(d), n = d->plan->n;
  if ((rc = solve_phase(d, d_arena, d_b, d_x, 0, st))) return rc;
  NCCLCHK(ncclAllReduce(d->ytmp + t0, d->ytmp + t0, (size_t)(n - t0), ncclDouble, ncclSum, c->comm, st));
  if ((rc = solve_phase(d, d_arena, d_b, d_x, 1, st))) return rc;
  NCCLCHK(ncclAllReduce(d->ytmp, d->ytmp, (size_t)n, ncclDouble, ncclSum, c->comm, st));
  return solve_phase(d, d_arena, d_b, d_x, 2, st);
}
extern "C" int cholamd_solve_sharded(cholamd_device *d, const double *d_arena, const double *d_b, double *d_x, cholamd_comm *c, void *stream)
{
  return solve_sharded_t<double>(d, d_arena, d_b, d_x, c, (hipStream_t)stream);
}
extern "C" int cholamd_solve_sharded_f32(cholamd_device *d, const float *d_arena32, const double *d_b, double *d_x, cholamd_comm *c, void *stream)
{
  return solve_sharded_t<float>(d, d_arena32, d_b, d_x, c, (hipStream_t)stream);
}
extern "C" int cholamd_solve_refine_sharded(cholamd_device *d, const float *d_arena32, const double *d_b, double *d_x, int max_iter, double tol,
                                            int *iters_out, double *relres_out, cholamd_comm *c, void *stream)
{ // every rank calls it with the same b; every rank ends with the same x, iteration count and residual
  HIPCHK(hipSetDevice(d->dev));
  int rc = ensure_refine(d);
  if (rc) return rc;
  const double *rv = d->rvec;
  double *dx = d->dxvec;
  return refine_loop(&d, 1, &d_b, &d_x, &rv, &dx, &stream, max_iter, tol, iters_out, relres_out,
                     [&](const double *const *r, double *const *o) { return solve_sharded_t<float>(d, d_arena32, r[0], o[0], c, (hipStream_t)stream); });
}
template <class TL> static int solve_multi_t(cholamd_device *const *devs, const TL *const *arenas, const double *const *bs, double *const *xs, cholamd_comm *const *comms,
                                             int n, void *const *streams)
{
  if (n < 1) { chol_set_error("no devices"); return CHOLAMD_ERR_ARG; }
  if (n == 1) { HIPCHK(hipSetDevice(devs[0]->dev)); return solve_t(devs[0], arenas[0], bs[0], xs[0], CHOL_BOTH_SWEEPS, stream_of(streams, 0)); }
  local_group *G = comms[0] ? comms[0]->local : nullptr;
  for (int g = 0; g < n; g++) {
    if (devs[g]->world != n || devs[g]->rank != g) { chol_set_error("device %d is not partitioned as rank %d of %d", g, g, n); return CHOLAMD_ERR_ARG; }
    if (comm_matches(devs[g], comms[g])) return CHOLAMD_ERR_ARG;
    if (comms[g]->local != G || (!G && !comms[g]->comm)) { chol_set_error("the %d communicators are not of one kind", n); return CHOLAMD_ERR_ARG; }
    HIPCHK(hipSetDevice(devs[g]->dev));
    int rc = build_solve(devs[g], g, n);
    if (rc) return rc;
  }
  const int64_t t0 = top_vec_offset(devs[0]), nn = devs[0]->plan->n;
  for (int ph = 0; ph < 3; ph++) {
    for (int g = 0; g < n; g++) {
      HIPCHK(hipSetDevice(devs[g]->dev));
      int rc = solve_phase(devs[g], arenas[g], bs[g], xs[g], ph, stream_of(streams, g));
      if (rc) return rc;
    }
    if (ph < 2) { int rc = multi_sum_vec(devs, comms, n, streams, ph == 0 ? t0 : 0, ph == 0 ? nn - t0 : nn); if (rc) return rc; }
  }
  return 0;
}
extern "C" int cholamd_solve_multi(cholamd_device *const *devs, const double *const *arenas, const double *const *bs, double *const *xs, cholamd_comm *const *comms,
                                   int n, void *const *streams)
{
  return solve_multi_t<double>(devs, arenas, bs, xs, comms, n, streams);
}
extern "C" int cholamd_solve_refine_multi(cholamd_device *const *devs, const float *const *arenas32, const double *const *bs, double *const *xs, int max_iter, double tol,
                                          int *iters_out, double *relres_out, cholamd_comm *const *comms, int n, void *const *streams)
{
  if (n < 1) { chol_set_error("no devices"); return CHOLAMD_ERR_ARG; }
  for (int g = 0; g < n; g++) { HIPCHK(hipSetDevice(devs[g]->dev)); int rc = ensure_refine(devs[g]); if (rc) return rc; }
  std::vector<const double *> rv(n);
  std::vector<double *> dx(n);
  for (int g = 0; g < n; g++) { rv[g] = devs[g]->rvec; dx[g] = devs[g]->dxvec; }
  return refine_loop(devs, n, bs, xs, rv.data(), dx.data(), streams, max_iter, tol, iters_out, relres_out,
                     [&](const double *const *r, double *const *o) { return solve_multi_t<float>(devs, arenas32, r, o, comms, n, streams); });
}

// the templates that other glue files call (chol_device.h), for the two element types of the arena: the sweeps (chol_api_schur.cpp) and the solves by the
// options in force (chol_api_pcg.cpp)
template int form_inverses<double>(cholamd_device *, const double *, int, bool, hipStream_t);
template int sweep_levels<double>(cholamd_device *, const double *, sweep_rhs, bool, int, int, int64_t *, hipStream_t);
template int sweep_steps<double>(cholamd_device *, const double *, const sdet_dev &, int, sweep_rhs, int64_t *, hipStream_t);
template int form_inverses<float>(cholamd_device *, const float *, int, bool, hipStream_t);
template int sweep_levels<float>(cholamd_device *, const float *, sweep_rhs, bool, int, int, int64_t *, hipStream_t);
template int sweep_steps<float>(cholamd_device *, const float *, const sdet_dev &, int, sweep_rhs, int64_t *, hipStream_t);
template int solve_any<double>(cholamd_device *, const double *, const double *, double *, int, hipStream_t);
template int solve_any<float>(cholamd_device *, const float *, const double *, double *, int, hipStream_t);
template int solve_nrhs_any<double>(cholamd_device *, const double *, const double *, int64_t, double *, int64_t, int, bool, int, hipStream_t);
template int solve_nrhs_any<float>(cholamd_device *, const float *, const double *, int64_t, double *, int64_t, int, bool, int, hipStream_t);
