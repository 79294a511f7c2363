// C ABI glue of libcholamd, low-rank corrections on a finished factor: updates, downdates and linear constraints through the public entry points of
// the device object they refer to.  Compiled with hipcc like chol_api.cpp; what they share is in chol_device.h.
#include "chol_device.h"

// ---------------------------------------------------------------------------------------------
// Low-rank corrections on the finished factor (include/cholamd.h at "low-rank corrections"; kernels in chol_lowrank.hip).  The object owns W = A^-1 U L_C^-T
// (n x kmax, leading dimension n), the capacitance factor C -> L_C and R = L_C^-T (kmax x kmax), two k x 32 blocks for t and the stage-1 workspace of
// the transposed product.  Everything else goes through the public entry points of the device object it refers to.
// ---------------------------------------------------------------------------------------------
struct cholamd_lowrank {
  cholamd_device *d = nullptr;
  int kmax = 0, k = 0, mode = 0, info = 0; // k == 0: unset
  int64_t ldw = 0;
  double logdet = 0.0;
  dev_buf<double> W, C, R, T, T2, ws;
  std::vector<double> LC; // L_C on the host (k x k, the upper triangle zero), read back by set
};
static int lowrank_rank_ok(const cholamd_device *d, const char *what)
{
  if (d->world > 1 && d->rank != 0) { chol_set_error("%s: rank %d of %d holds no complete factor (gather to rank 0 and use its device object)", what, d->rank, d->world); return CHOLAMD_ERR_ARG; }
  return 0;
}
static int lowrank_is_set(const cholamd_lowrank *lr, const char *what)
{
  if (!lr) { chol_set_error("%s: NULL object", what); return CHOLAMD_ERR_ARG; }
  if (lr->k <= 0) { chol_set_error("%s: the object is unset (no successful cholamd_lowrank_set)", what); return CHOLAMD_ERR_ARG; }
  return 0;
}
extern "C" int cholamd_lowrank_create(cholamd_device *d, int kmax, cholamd_lowrank **out)
{
  const char *what = "cholamd_lowrank_create";
  if (out) *out = nullptr;
  if (!d || !out) { chol_set_error("%s: NULL %s", what, !d ? "device" : "out"); return CHOLAMD_ERR_ARG; }
  if (kmax < 1 || kmax > CHOLAMD_LOWRANK_MAX) { chol_set_error("%s: kmax = %d is not in 1 .. %d", what, kmax, CHOLAMD_LOWRANK_MAX); return CHOLAMD_ERR_ARG; }
  { int rc = lowrank_rank_ok(d, what); if (rc) return rc; }
  HIPCHK(hipSetDevice(d->dev));
  cholamd_lowrank *lr = new cholamd_lowrank;
  lr->d = d; lr->kmax = kmax; lr->ldw = d->plan->n;
  const size_t n = (size_t)d->plan->n, kk = (size_t)kmax * kmax, kt = (size_t)kmax * CHOL_NRHS_W;
  int rc = lr->W.alloc(n * kmax);
  if (!rc) rc = lr->C.alloc(kk);
  if (!rc) rc = lr->R.alloc(kk);
  if (!rc) rc = lr->T.alloc(kt);
  if (!rc) rc = lr->T2.alloc(kt);
  if (!rc) rc = lr->ws.alloc((size_t)chol_lr_ws_doubles(d->plan->n, kmax));
  if (rc) { delete lr; return rc; }
  *out = lr;
  return 0;
}
extern "C" void cholamd_lowrank_destroy(cholamd_lowrank *lr) { delete lr; }
extern "C" int cholamd_lowrank_state(const cholamd_lowrank *lr, int out[3])
{
  if (!lr || !out) { chol_set_error("cholamd_lowrank_state: NULL %s", !lr ? "object" : "out"); return CHOLAMD_ERR_ARG; }
  out[0] = lr->k; out[1] = lr->mode; out[2] = lr->info;
  return 0;
}
extern "C" int cholamd_lowrank_set(cholamd_lowrank *lr, const double *d_arena, const double *d_U, int64_t ldu, int k, int mode, void *stream)
{
  const char *what = "cholamd_lowrank_set";
  hipStream_t st = (hipStream_t)stream;
  if (!lr) { chol_set_error("%s: NULL object", what); return CHOLAMD_ERR_ARG; }
  cholamd_device *d = lr->d;
  const int n = d->plan->n, kmax = lr->kmax;
  if (!d_arena || !d_U) { chol_set_error("%s: NULL %s", what, !d_arena ? "arena" : "U"); return CHOLAMD_ERR_ARG; }
  if (k < 1 || k > kmax) { chol_set_error("%s: k = %d is not in 1 .. kmax = %d", what, k, kmax); return CHOLAMD_ERR_ARG; }
  if (ldu < n) { chol_set_error("%s: ldu = %lld must be at least n = %d", what, (long long)ldu, n); return CHOLAMD_ERR_ARG; }
  if (mode != CHOLAMD_LOWRANK_UPDATE && mode != CHOLAMD_LOWRANK_DOWNDATE && mode != CHOLAMD_LOWRANK_CONSTRAINT) {
    chol_set_error("%s: mode = %d is none of CHOLAMD_LOWRANK_UPDATE (1), _DOWNDATE (-1), _CONSTRAINT (0)", what, mode);
    return CHOLAMD_ERR_ARG;
  }
  { int rc = lowrank_rank_ok(d, what); if (rc) return rc; }
  HIPCHK(hipSetDevice(d->dev));
  lr->k = 0; lr->mode = mode; lr->info = 0;
  double *W = lr->W, *C = lr->C, *R = lr->R;
  const int64_t ldw = lr->ldw;
  HIPCHK(hipMemcpy2DAsync(W, (size_t)ldw * sizeof(double), d_U, (size_t)ldu * sizeof(double), (size_t)n * sizeof(double), (size_t)k, hipMemcpyDeviceToDevice, st));
  { int rc = cholamd_solve_half_nrhs(d, d_arena, W, ldw, W, ldw, k, CHOLAMD_HALF_FORWARD, st); if (rc) return rc; }         // Y = M^-1 U
  HIPCHK((hipError_t)chol_launch_lr_tprod(n, k, k, W, ldw, W, ldw, lr->ws, C, kmax, st));                                   // G = Y^T Y
  HIPCHK((hipError_t)chol_launch_lr_small(0, k, k, mode, C, kmax, nullptr, 0, st));                                         // C = I +- G, or G
  const int info = cholamd_dpotrf_dev(k, C, kmax, nullptr, st);                                                             // C = L_C L_C^T (synchronises)
  if (info < 0) return info;
  if (info > 0) {
    lr->info = info;
    chol_set_error("%s: the capacitance matrix %s is not positive definite at leading minor %d%s", what, mode > 0 ? "I + U^T A^-1 U" : mode < 0 ? "I - U^T A^-1 U" : "U^T A^-1 U", info,
                   mode < 0 ? " (A - U U^T is not positive definite)" : mode == 0 ? " (the constraint columns are dependent or zero)" : "");
    return CHOLAMD_ERR_ARG;
  }
  { int rc = cholamd_solve_half_nrhs(d, d_arena, W, ldw, W, ldw, k, CHOLAMD_HALF_BACKWARD, st); if (rc) return rc; }        // V = M^-T Y
  HIPCHK((hipError_t)chol_launch_lr_small(1, k, k, 0, R, kmax, nullptr, 0, st));
  { int rc = cholamd_dtrsm_dev(k, k, C, kmax, R, kmax, st); if (rc) return rc; }                                            // R = I L_C^-T
  HIPCHK((hipError_t)chol_launch_lr_rprod(n, k, k, 0.0, 1.0, W, ldw, R, kmax, W, ldw, st));                                 // W = V R, in place
  lr->LC.assign((size_t)k * k, 0.0);
  HIPCHK(hipMemcpy2DAsync(lr->LC.data(), (size_t)k * sizeof(double), C, (size_t)kmax * sizeof(double), (size_t)k * sizeof(double), (size_t)k, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  double sum = 0.0;
  for (int j = 0; j < k; j++) {
    for (int i = 0; i < j; i++) lr->LC[i + (size_t)j * k] = 0.0;
    sum += std::log(lr->LC[j + (size_t)j * k]);
  }
  lr->logdet = 2.0 * sum;
  lr->k = k;
  return 0;
}
// t (k x cols, leading dimension kmax, in lr->T) of one chunk: W^T B, in constraint mode minus L_C^-1 E = R^T E
static int lowrank_t(cholamd_lowrank *lr, const double *B, int64_t ldb, const double *E, int64_t lde, int cols, hipStream_t st)
{
  const int n = lr->d->plan->n, k = lr->k, kmax = lr->kmax;
  HIPCHK((hipError_t)chol_launch_lr_tprod(n, k, cols, lr->W, lr->ldw, B, ldb, lr->ws, lr->T, kmax, st));
  if (lr->mode == CHOLAMD_LOWRANK_CONSTRAINT && E) {
    HIPCHK((hipError_t)chol_launch_lr_tprod(k, k, cols, lr->R, kmax, E, lde, lr->ws, lr->T2, kmax, st));
    HIPCHK((hipError_t)chol_launch_lr_small(2, k, cols, 0, lr->T, kmax, lr->T2, kmax, st));
  }
  return 0;
}
static double lowrank_sigma(const cholamd_lowrank *lr) { return lr->mode == CHOLAMD_LOWRANK_DOWNDATE ? -1.0 : 1.0; }
extern "C" int cholamd_lowrank_solve(cholamd_lowrank *lr, const double *d_arena, const double *d_b, const double *d_e, double *d_x, void *stream)
{
  const char *what = "cholamd_lowrank_solve";
  hipStream_t st = (hipStream_t)stream;
  { int rc = lowrank_is_set(lr, what); if (rc) return rc; }
  if (!d_arena || !d_b || !d_x) { chol_set_error("%s: NULL %s", what, !d_arena ? "arena" : !d_b ? "b" : "x"); return CHOLAMD_ERR_ARG; }
  cholamd_device *d = lr->d;
  const int n = d->plan->n;
  { int rc = lowrank_rank_ok(d, what); if (rc) return rc; }
  HIPCHK(hipSetDevice(d->dev));
  { int rc = lowrank_t(lr, d_b, n, d_e, lr->k, 1, st); if (rc) return rc; }
  { int rc = cholamd_solve(d, d_arena, d_b, d_x, st); if (rc) return rc; }
  HIPCHK((hipError_t)chol_launch_lr_rprod(n, lr->k, 1, 1.0, -lowrank_sigma(lr), lr->W, lr->ldw, lr->T, lr->kmax, d_x, n, st));
  return 0;
}
extern "C" int cholamd_lowrank_solve_nrhs(cholamd_lowrank *lr, const double *d_arena, const double *d_B, int64_t ldb, const double *d_E, int64_t lde, double *d_X, int64_t ldx, int nrhs,
                                          void *stream)
{
  const char *what = "cholamd_lowrank_solve_nrhs";
  hipStream_t st = (hipStream_t)stream;
  { int rc = lowrank_is_set(lr, what); if (rc) return rc; }
  cholamd_device *d = lr->d;
  { int rc = nrhs_check(d, d_arena, d_B, ldb, d_X, ldx, nrhs, what); if (rc) return rc > 0 ? 0 : rc; }
  const bool with_e = lr->mode == CHOLAMD_LOWRANK_CONSTRAINT && d_E;
  if (with_e && lde < lr->k) { chol_set_error("%s: lde = %lld must be at least k = %d", what, (long long)lde, lr->k); return CHOLAMD_ERR_ARG; }
  { int rc = lowrank_rank_ok(d, what); if (rc) return rc; }
  HIPCHK(hipSetDevice(d->dev));
  const int n = d->plan->n;
  for (int c0 = 0; c0 < nrhs; c0 += CHOL_NRHS_W) {
    const int cols = std::min(CHOL_NRHS_W, nrhs - c0);
    const double *B = d_B + (int64_t)c0 * ldb;
    double *X = d_X + (int64_t)c0 * ldx;
    { int rc = lowrank_t(lr, B, ldb, with_e ? d_E + (int64_t)c0 * lde : nullptr, lde, cols, st); if (rc) return rc; }
    { int rc = cholamd_solve_nrhs(d, d_arena, B, ldb, X, ldx, cols, st); if (rc) return rc; }
    HIPCHK((hipError_t)chol_launch_lr_rprod(n, lr->k, cols, 1.0, -lowrank_sigma(lr), lr->W, lr->ldw, lr->T, lr->kmax, X, ldx, st));
  }
  return 0;
}
extern "C" int cholamd_lowrank_project(cholamd_lowrank *lr, const double *d_U, int64_t ldu, const double *d_x, const double *d_e, double *d_xout, void *stream)
{
  const char *what = "cholamd_lowrank_project";
  hipStream_t st = (hipStream_t)stream;
  { int rc = lowrank_is_set(lr, what); if (rc) return rc; }
  cholamd_device *d = lr->d;
  const int n = d->plan->n, k = lr->k, kmax = lr->kmax;
  if (lr->mode != CHOLAMD_LOWRANK_CONSTRAINT) { chol_set_error("%s: the object is not in constraint mode", what); return CHOLAMD_ERR_ARG; }
  if (!d_U || !d_x || !d_xout) { chol_set_error("%s: NULL %s", what, !d_U ? "U" : !d_x ? "x" : "xout"); return CHOLAMD_ERR_ARG; }
  if (ldu < n) { chol_set_error("%s: ldu = %lld must be at least n = %d", what, (long long)ldu, n); return CHOLAMD_ERR_ARG; }
  HIPCHK(hipSetDevice(d->dev));
  HIPCHK((hipError_t)chol_launch_lr_tprod(n, k, 1, d_U, ldu, d_x, n, lr->ws, lr->T, kmax, st));                   // U^T x
  if (d_e) HIPCHK((hipError_t)chol_launch_lr_small(2, k, 1, 0, lr->T, kmax, d_e, k, st));                        // - e
  HIPCHK((hipError_t)chol_launch_lr_tprod(k, k, 1, lr->R, kmax, lr->T, kmax, lr->ws, lr->T2, kmax, st));          // L_C^-1 (U^T x - e)
  if (d_xout != d_x) HIPCHK(hipMemcpyAsync(d_xout, d_x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIPCHK((hipError_t)chol_launch_lr_rprod(n, k, 1, 1.0, -1.0, lr->W, lr->ldw, lr->T2, kmax, d_xout, n, st));
  return 0;
}
extern "C" int cholamd_lowrank_diag(cholamd_lowrank *lr, double *d_w, void *stream)
{
  const char *what = "cholamd_lowrank_diag";
  { int rc = lowrank_is_set(lr, what); if (rc) return rc; }
  if (!d_w) { chol_set_error("%s: NULL w", what); return CHOLAMD_ERR_ARG; }
  HIPCHK(hipSetDevice(lr->d->dev));
  HIPCHK((hipError_t)chol_launch_lr_rowsq(lr->d->plan->n, lr->k, lr->W, lr->ldw, d_w, (hipStream_t)stream));
  return 0;
}
extern "C" int cholamd_lowrank_logdet(cholamd_lowrank *lr, double *logdet_C_out)
{
  const char *what = "cholamd_lowrank_logdet";
  { int rc = lowrank_is_set(lr, what); if (rc) return rc; }
  if (!logdet_C_out) { chol_set_error("%s: NULL logdet_C_out", what); return CHOLAMD_ERR_ARG; }
  *logdet_C_out = lr->logdet;
  return 0;
}
extern "C" int cholamd_lowrank_factor(cholamd_lowrank *lr, double *h_LC, int ldl)
{
  const char *what = "cholamd_lowrank_factor";
  { int rc = lowrank_is_set(lr, what); if (rc) return rc; }
  if (!h_LC || ldl < lr->k) { chol_set_error("%s: %s", what, !h_LC ? "NULL h_LC" : "ldl < k"); return CHOLAMD_ERR_ARG; }
  for (int j = 0; j < lr->k; j++) std::memcpy(h_LC + (size_t)j * ldl, lr->LC.data() + (size_t)j * lr->k, (size_t)lr->k * sizeof(double));
  return 0;
}
extern "C" int cholamd_lowrank_block(cholamd_lowrank *lr, const double **d_W, int64_t *ldw)
{
  const char *what = "cholamd_lowrank_block";
  { int rc = lowrank_is_set(lr, what); if (rc) return rc; }
  if (!d_W || !ldw) { chol_set_error("%s: NULL %s", what, !d_W ? "d_W" : "ldw"); return CHOLAMD_ERR_ARG; }
  *d_W = lr->W; *ldw = lr->ldw;
  return 0;
}
