// C ABI glue of libcholamd: y = A x and the preconditioned conjugate gradients.  Compiled with hipcc like chol_api.cpp; what they share is in
// chol_device.h.
#include "chol_device.h"

// ---------------------------------------------------------------------------------------------
// y = A x with the values in force, and conjugate gradients on A preconditioned with the factor in the arena (include/cholamd.h at cholamd_solve_pcg;
// kernels in chol_pcg.hip).  The factor may be that of other values on the pattern, or of lower precision: M = L L^T only has to be SPD.
// ---------------------------------------------------------------------------------------------
extern "C" int cholamd_apply_nrhs(cholamd_device *d, const double *d_X, int64_t ldx, double *d_Y, int64_t ldy, int nrhs, void *stream)
{
  { int rc = block_check(d, false, nullptr, d_X, ldx, d_Y, ldy, nrhs, "cholamd_apply_nrhs", "X", "Y"); if (rc) return rc > 0 ? 0 : rc; }
  const int n = d->plan->n;
  if (ranges_overlap(d_X, ((size_t)(nrhs - 1) * ldx + n) * sizeof(double), d_Y, ((size_t)(nrhs - 1) * ldy + n) * sizeof(double))) {
    chol_set_error("cholamd_apply_nrhs: Y overlaps X (there is no in-place form)");
    return CHOLAMD_ERR_ARG;
  }
  HIPCHK(hipSetDevice(d->dev));
  { int rc = ensure_csr(d); if (rc) return rc; }
  for (int c0 = 0; c0 < nrhs; c0 += CHOL_NRHS_W)
    HIPCHK((hipError_t)chol_launch_pcg_apply(d->csr_ptr, d->csr_col, d->csr_val, d_X + (int64_t)c0 * ldx, ldx, d_Y + (int64_t)c0 * ldy, ldy, n, std::min(CHOL_NRHS_W, nrhs - c0),
                                             nullptr, (hipStream_t)stream));
  return 0;
}
extern "C" int cholamd_apply(cholamd_device *d, const double *d_x, double *d_y, void *stream)
{
  if (!d || !d_x || !d_y) { chol_set_error("cholamd_apply: NULL %s", !d ? "device" : !d_x ? "x" : "y"); return CHOLAMD_ERR_ARG; }
  const int n = d->plan->n;
  if (ranges_overlap(d_x, (size_t)n * sizeof(double), d_y, (size_t)n * sizeof(double))) { chol_set_error("cholamd_apply: y overlaps x (there is no in-place form)"); return CHOLAMD_ERR_ARG; }
  HIPCHK(hipSetDevice(d->dev));
  { int rc = ensure_csr(d); if (rc) return rc; }
  HIPCHK((hipError_t)chol_launch_pcg_apply(d->csr_ptr, d->csr_col, d->csr_val, d_x, n, d_y, n, n, 1, nullptr, (hipStream_t)stream));
  return 0;
}
// the columns' records on the host: one copy and one synchronisation of the stream
static int pcg_read(cholamd_device *d, int cols, chol_pcg_rec *h, hipStream_t st)
{
  HIPCHK(hipMemcpyAsync(d->pcg_host, d->pcg_rec, (size_t)cols * sizeof(chol_pcg_rec), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::memcpy(h, d->pcg_host, (size_t)cols * sizeof(chol_pcg_rec));
  return 0;
}
// The loop, chunk by chunk of CHOL_NRHS_W columns.  single: the one-vector entry points, whose M^-1 is cholamd_solve's (solve_any); otherwise
// cholamd_solve_nrhs's (solve_nrhs_any).  Per iteration and chunk: z = M^-1 r | rho = r^T z, beta | p = z + beta p | q = A p, sigma = p^T q, alpha |
// x += alpha p, r -= alpha q, rr = ||r||^2 | one read-back of the records.  All scalars stay on the device; the host only reads the states.
template <class TL> static int pcg_t(cholamd_device *d, const TL *d_arena, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, int max_iter, double tol, int flags,
                                     int *iters_out, double *relres_out, int *status_out, bool single, hipStream_t st, const char *what)
{
  { int rc = nrhs_check(d, d_arena, d_B, ldb, d_X, ldx, nrhs, what, single ? "b" : "B", single ? "x" : "X"); if (rc) return rc > 0 ? 0 : rc; }
  if (flags < 0 || (flags & ~CHOLAMD_PCG_X0)) { chol_set_error("%s: bad flags %d", what, flags); return CHOLAMD_ERR_ARG; }
  if (!(tol >= 0.0) || std::isinf(tol)) { chol_set_error("%s: tol = %g is not a finite number >= 0", what, tol); return CHOLAMD_ERR_ARG; }
  if (d->world > 1 && d->rank != 0) {
    chol_set_error("%s: rank %d of %d holds its own subtrees only; the call needs the complete factor (a single-GPU object, or rank 0 after a gather)", what, d->rank, d->world);
    return CHOLAMD_ERR_ARG;
  }
  HIPCHK(hipSetDevice(d->dev));
  const int n = d->plan->n, nb = (n + 255) / 256;
  const size_t blk = (size_t)(n > 0 ? n : 1) * CHOL_NRHS_W;
  int rc = ensure_refine(d);
  if (!rc) rc = build_solve(d);
  if (!rc) rc = d->rnrhs.ensure(blk);
  if (!rc) rc = d->pnrhs.ensure((size_t)2 * (nb > 0 ? nb : 1) * CHOL_NRHS_W);
  if (!rc) rc = d->pcg_b.ensure(blk);
  if (!rc) rc = d->pcg_p.ensure(blk);
  if (!rc) rc = d->pcg_q.ensure(blk);
  if (!rc) rc = d->pcg_r.ensure(blk);
  if (!rc) rc = d->pcg_z.ensure(blk);
  if (!rc) rc = d->pcg_part.ensure((size_t)(nb > 0 ? nb : 1) * CHOL_NRHS_W);
  if (!rc) rc = d->pcg_rec.ensure_zero(CHOL_NRHS_W);
  if (!rc) rc = d->pcg_host.ensure((CHOL_NRHS_W * sizeof(chol_pcg_rec) + 7) / 8);
  if (rc) return rc;
  if (max_iter < 0) max_iter = 0;
  keep_inverses_scope keep(&d, 1);
  d->keep_inverses = false; // (until the first solve has formed them)
  double *const Bw = d->pcg_b, *const P = d->pcg_p, *const Q = d->pcg_q, *const R = d->pcg_r, *const Z = d->pcg_z, *const T = d->rnrhs;
  chol_pcg_rec h[CHOL_NRHS_W];
  int bad_col = -1; chol_pcg_rec bad = {};
  auto live = [&](int cols) { for (int j = 0; j < cols; j++) if (h[j].state == CHOL_PCG_RUNNING || h[j].state == CHOL_PCG_RESTART) return true; return false; };
  auto true_residual = [&](double *X, int cols, int stage) { // T = b - A x for the chunk, the records moved on by `stage`
    hipError_t e = (hipError_t)chol_nrhs_launch_residual(d->csr_ptr, d->csr_col, d->csr_val, Bw, n, X, ldx, T, n, n, cols, d->pnrhs, st);
    return e != hipSuccess ? e : (hipError_t)chol_launch_pcg_scalars(d->pcg_rec, d->pnrhs, n, cols, stage, tol, st);
  };
  for (int c0 = 0; c0 < nrhs; c0 += CHOL_NRHS_W) {
    const int cols = std::min(CHOL_NRHS_W, nrhs - c0);
    double *X = d_X + (int64_t)c0 * ldx;
    // the chunk's columns of B first (X may be B), then the start: x = 0 unless the caller's x is the start vector, r = b - A x with its norm and b's
    HIPCHK(hipMemcpy2DAsync(Bw, (size_t)n * sizeof(double), d_B + (int64_t)c0 * ldb, (size_t)ldb * sizeof(double), (size_t)n * sizeof(double), (size_t)cols, hipMemcpyDeviceToDevice, st));
    if (!(flags & CHOLAMD_PCG_X0)) HIPCHK(hipMemset2DAsync(X, (size_t)ldx * sizeof(double), 0, (size_t)n * sizeof(double), (size_t)cols, st));
    HIPCHK((hipError_t)chol_nrhs_launch_residual(d->csr_ptr, d->csr_col, d->csr_val, Bw, n, X, ldx, R, n, n, cols, d->pnrhs, st));
    HIPCHK((hipError_t)chol_launch_pcg_scalars(d->pcg_rec, d->pnrhs, n, cols, CHOL_PCG_STAGE_INIT, tol, st));
    if ((rc = pcg_read(d, cols, h, st))) return rc;
    if (flags & CHOLAMD_PCG_X0)
      for (int j = 0; j < cols; j++) // b = 0: x = 0, whatever the start vector was
        if (h[j].state == CHOL_PCG_ZERO_B) HIPCHK(hipMemsetAsync(X + (int64_t)j * ldx, 0, (size_t)n * sizeof(double), st));
    for (int it = 0; it < max_iter && live(cols); it++) {
      rc = single ? solve_any(d, d_arena, R, Z, CHOL_BOTH_SWEEPS, st) : solve_nrhs_any(d, d_arena, R, n, Z, n, cols, false, CHOL_BOTH_SWEEPS, st);
      if (rc) return rc;
      d->keep_inverses = true;
      HIPCHK((hipError_t)chol_launch_pcg_dot(R, Z, n, n, cols, d->pcg_part, st));
      HIPCHK((hipError_t)chol_launch_pcg_scalars(d->pcg_rec, d->pcg_part, n, cols, CHOL_PCG_STAGE_RHO, tol, st));
      HIPCHK((hipError_t)chol_launch_pcg_direction(d->pcg_rec, Z, P, n, n, cols, st));
      HIPCHK((hipError_t)chol_launch_pcg_apply(d->csr_ptr, d->csr_col, d->csr_val, P, n, Q, n, n, cols, d->pcg_part, st));
      HIPCHK((hipError_t)chol_launch_pcg_scalars(d->pcg_rec, d->pcg_part, n, cols, CHOL_PCG_STAGE_SIGMA, tol, st));
      HIPCHK((hipError_t)chol_launch_pcg_update(d->pcg_rec, P, Q, X, ldx, R, n, n, cols, d->pcg_part, st));
      HIPCHK((hipError_t)chol_launch_pcg_scalars(d->pcg_rec, d->pcg_part, n, cols, CHOL_PCG_STAGE_RR, tol, st));
      if ((rc = pcg_read(d, cols, h, st))) return rc;
      bool claim = false;
      for (int j = 0; j < cols; j++) claim |= h[j].state == CHOL_PCG_CLAIM;
      if (!claim) continue;
      // a column claims rr <= tol^2 bb by the recurrence: the true residual decides; where it does not agree it becomes r and the column runs on with p = z
      HIPCHK(true_residual(X, cols, CHOL_PCG_STAGE_VERIFY));
      HIPCHK((hipError_t)chol_launch_pcg_take(d->pcg_rec, T, R, n, n, cols, st));
      if ((rc = pcg_read(d, cols, h, st))) return rc;
    }
    bool all_conv = true;
    for (int j = 0; j < cols; j++) all_conv &= h[j].state == CHOL_PCG_CONVERGED || h[j].state == CHOL_PCG_ZERO_B;
    if (!all_conv) { // relres is the true residual of what is returned, also where the loop gave up
      HIPCHK(true_residual(X, cols, CHOL_PCG_STAGE_FINAL));
      if ((rc = pcg_read(d, cols, h, st))) return rc;
    }
    for (int j = 0; j < cols; j++) {
      const int s = h[j].state;
      const int status = s == CHOL_PCG_CONVERGED || s == CHOL_PCG_ZERO_B ? CHOL_PCG_CONVERGED : s == CHOL_PCG_BREAKDOWN || s == CHOL_PCG_NAN ? s : CHOL_PCG_MAXITER;
      if (iters_out) iters_out[c0 + j] = h[j].iters;
      if (relres_out) relres_out[c0 + j] = h[j].rel;
      if (status_out) status_out[c0 + j] = status;
      if (status >= CHOL_PCG_BREAKDOWN && bad_col < 0) { bad_col = c0 + j; bad = h[j]; }
    }
  }
  if (bad_col < 0) return 0;
  if (bad.state == CHOL_PCG_NAN) chol_set_error("%s: column %d produced NaN or inf (status 3: the right-hand side, the values in force or the factor are not finite)", what, bad_col);
  else chol_set_error("%s: column %d broke down after %d iterations: %s = %.17g <= 0 (status 2: the values in force are not positive definite, or the factor is broken); x keeps the last iterate",
                      what, bad_col, bad.iters, bad.what == 1 ? "r^T M^-1 r" : "p^T A p", bad.what == 1 ? bad.rho : bad.sigma);
  return CHOLAMD_ERR_ARG;
}
extern "C" int cholamd_solve_pcg(cholamd_device *d, const double *d_arena, const double *d_b, double *d_x, int max_iter, double tol, int flags,
                                 int *iters_out, double *relres_out, int *status_out, void *stream)
{ return pcg_t(d, d_arena, d_b, d ? d->plan->n : 0, d_x, d ? d->plan->n : 0, 1, max_iter, tol, flags, iters_out, relres_out, status_out, true, (hipStream_t)stream, "cholamd_solve_pcg"); }
extern "C" int cholamd_solve_pcg_f32(cholamd_device *d, const float *d_arena32, const double *d_b, double *d_x, int max_iter, double tol, int flags,
                                     int *iters_out, double *relres_out, int *status_out, void *stream)
{ return pcg_t(d, d_arena32, d_b, d ? d->plan->n : 0, d_x, d ? d->plan->n : 0, 1, max_iter, tol, flags, iters_out, relres_out, status_out, true, (hipStream_t)stream, "cholamd_solve_pcg_f32"); }
extern "C" int cholamd_solve_pcg_nrhs(cholamd_device *d, const double *d_arena, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, int max_iter, double tol, int flags,
                                      int *iters_out, double *relres_out, int *status_out, void *stream)
{ return pcg_t(d, d_arena, d_B, ldb, d_X, ldx, nrhs, max_iter, tol, flags, iters_out, relres_out, status_out, false, (hipStream_t)stream, "cholamd_solve_pcg_nrhs"); }
extern "C" int cholamd_solve_pcg_nrhs_f32(cholamd_device *d, const float *d_arena32, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int nrhs, int max_iter, double tol, int flags,
                                          int *iters_out, double *relres_out, int *status_out, void *stream)
{ return pcg_t(d, d_arena32, d_B, ldb, d_X, ldx, nrhs, max_iter, tol, flags, iters_out, relres_out, status_out, false, (hipStream_t)stream, "cholamd_solve_pcg_nrhs_f32"); }
