// C ABI glue of libcholamd, the Schur complement on the top levels of the tree: the partial factor, the gather of S, condense and expand for one
// vector and for blocks, atomic or deterministic.  Compiled with hipcc like chol_api.cpp; it composes the sweep helpers of chol_api_solve.cpp (chol_device.h).
#include "chol_device.h"

// ---------------------------------------------------------------------------------------------
// Schur complement on the top k levels of the tree (include/cholamd.h at cholamd_schur; the gather kernel in chol_schur.hip).  The factorisation is
// right-looking: after the levels levels - 1 .. k every contribution of the eliminated separators sits in the blocks of the kept ones, which then hold
// S = A_TT - A_TI A_II^-1 A_IT.  Condense and expand are the streamed solve cut at level k instead of at the partition's level: the same launches over
// a level range, the levels above the cut never read as a factor.
// ---------------------------------------------------------------------------------------------
// the checks every Schur entry point shares; returns m (the kept dofs) and *t0 = n - m, or the error
static int schur_args(const cholamd_device *d, int k, const char *what, int *t0)
{
  if (!d) { chol_set_error("%s: NULL device", what); return CHOLAMD_ERR_ARG; }
  if (d->world > 1) { chol_set_error("%s: the device object is partitioned (rank %d of %d); there are no sharded variants", what, d->rank, d->world); return CHOLAMD_ERR_ARG; }
  return chol_schur_range(d->plan, k, t0);
}
extern "C" int cholamd_schur_factor(cholamd_device *d, double *d_arena, int k, void *stream)
{
  const int m = schur_args(d, k, "cholamd_schur_factor", nullptr);
  if (m < 0) return m;
  if (!d_arena) { chol_set_error("cholamd_schur_factor: NULL arena"); return CHOLAMD_ERR_ARG; }
  return cholamd_factor_levels(d, d_arena, d->plan->levels - 1, k, stream); // the per-level launches, never the program
}
static int build_schur(cholamd_device *d, int k)
{
  if (d->sc.empty()) d->sc.resize(d->plan->levels);
  schur_dev &q = d->sc[k];
  if (q.n >= 0) return 0;
  const int64_t cnt = chol_schur_pieces(d->plan, k, 1, CHOL_SCHUR_CHUNK, 0, nullptr);
  if (cnt < 0) return (int)cnt;
  std::vector<chol_schur_desc> h((size_t)cnt);
  chol_schur_pieces(d->plan, k, 1, CHOL_SCHUR_CHUNK, cnt, h.data());
  int rc = q.desc.upload(h.data(), (size_t)cnt);
  if (rc) return rc;
  q.n = cnt;
  return 0;
}
extern "C" int cholamd_schur(cholamd_device *d, const double *d_arena, int k, double *d_S, int64_t lds, void *stream)
{
  const int m = schur_args(d, k, "cholamd_schur", nullptr);
  if (m < 0) return m;
  if (!d_arena || !d_S) { chol_set_error("cholamd_schur: NULL %s", !d_arena ? "arena" : "S"); return CHOLAMD_ERR_ARG; }
  if (lds < m) { chol_set_error("cholamd_schur: lds = %lld < m = %d", (long long)lds, m); return CHOLAMD_ERR_ARG; }
  if (m == 0) return 0;
  if (ranges_overlap(d_S, ((size_t)(m - 1) * (size_t)lds + (size_t)m) * sizeof(double), d_arena, (size_t)d->plan->arena * sizeof(double))) {
    chol_set_error("cholamd_schur: S overlaps the arena");
    return CHOLAMD_ERR_ARG;
  }
  HIPCHK(hipSetDevice(d->dev));
  { int rc = build_schur(d, k); if (rc) return rc; }
  HIPCHK((hipError_t)chol_launch_schur_gather(d_arena, d->sc[k].desc, d->sc[k].n, d_S, lds, (hipStream_t)stream));
  return 0;
}
// ---- option schur_deterministic: the step lists cut at k (chol_build_schur_det), per (device object, k), built at the first such call and kept
static int build_schur_det(cholamd_device *d, int k)
{
  if (d->scd.empty()) d->scd.resize(d->plan->levels);
  if (d->scd[k].ready) return 0;
  chol_sdet_lists w;
  int rc = chol_build_schur_det(d->plan, k, &w);
  if (rc) return rc;
  rc = upload_sdet(d->scd[k], w);
  chol_sdet_lists_free(&w);
  return rc;
}
// Condense, expand and their block forms by the one option they read, through the three helpers below:
//   schur_deterministic -> the step lists cut at k (sweep_steps), the 16x16 inverses of the levels under the cut alone; every chunk of a block takes them
//   otherwise           -> the atomic kernels over the levels k .. levels - 1 (sweep_levels), the span inverses too; a chunk of a block under
//                          half_nrhs_min_block goes column by column through the single-vector body
// The levels above the cut hold S, not a factor: no inverse is formed there.  Every launch is counted in schur_launches.
static int schur_build(cholamd_device *d, int k)
{
  int rc = build_solve(d);
  if (!rc && d->schur_deterministic) rc = build_schur_det(d, k);
  return rc;
}
template <class TL> static int schur_inverses(cholamd_device *d, const TL *d_arena, int k, hipStream_t st) { return form_inverses(d, d_arena, k, !d->schur_deterministic, st); }
template <class TL> static int schur_sweep(cholamd_device *d, const TL *d_arena, int k, bool backward, sweep_rhs rhs, hipStream_t st)
{
  return d->schur_deterministic ? sweep_steps(d, d_arena, d->scd[k], backward ? CHOLAMD_HALF_BACKWARD : CHOLAMD_HALF_FORWARD, rhs, d->schur_launches, st)
                                : sweep_levels(d, d_arena, rhs, backward, k, d->plan->levels - 1, &d->schur_launches[0], st);
}
// the single-vector bodies behind the checks (t0, m: chol_schur_range): the forward sweep under the cut in w, whose tail is g in Schur order ...
template <class TL> static int schur_condense_t(cholamd_device *d, const TL *d_arena, int k, int t0, int m, const double *d_b, double *d_w, double *d_g, hipStream_t st)
{
  { int rc = schur_build(d, k); if (rc) return rc; }
  const int n = d->plan->n;
  HIPCHK((hipError_t)chol_launch_permute(d_b, d->perm, d_w, n, 0, st));
  if (!d->keep_inverses) { int rc = schur_inverses(d, d_arena, k, st); if (rc) return rc; } // (kept: the column-by-column chunks of the block form)
  { int rc = schur_sweep(d, d_arena, k, false, { d_w, false }, st); if (rc) return rc; }
  if (m > 0) HIPCHK(hipMemcpyAsync(d_g, d_w + t0, (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, st));
  return 0;
}
// ... and the backward sweep under the cut from (w under the cut, xt above it); w stays as it is: the sweep runs in the device object's work vector
template <class TL> static int schur_expand_t(cholamd_device *d, const TL *d_arena, int k, int t0, int m, const double *d_w, const double *d_xt, double *d_x, hipStream_t st)
{
  { int rc = schur_build(d, k); if (rc) return rc; }
  const int n = d->plan->n;
  double *y = d->ytmp;
  if (t0 > 0) HIPCHK(hipMemcpyAsync(y, d_w, (size_t)t0 * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (m > 0) HIPCHK(hipMemcpyAsync(y + t0, d_xt, (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (!d->keep_inverses) { int rc = schur_inverses(d, d_arena, k, st); if (rc) return rc; } // as at the start of every half solve: the arena of the call before may have been another
  { int rc = schur_sweep(d, d_arena, k, true, { y, false }, st); if (rc) return rc; }
  HIPCHK((hipError_t)chol_launch_permute(y, d->perm, d_x, n, 1, st));
  return 0;
}
template <class TL> static int schur_condense_api(cholamd_device *d, const TL *d_arena, int k, const double *d_b, double *d_w, double *d_g, hipStream_t st, const char *what)
{
  int t0 = 0;
  const int m = schur_args(d, k, what, &t0);
  if (m < 0) return m;
  if (!d_arena || !d_b || !d_w || !d_g) { chol_set_error("%s: NULL %s", what, !d_arena ? "arena" : !d_b ? "b" : !d_w ? "w" : "g"); return CHOLAMD_ERR_ARG; }
  const size_t nb = (size_t)d->plan->n * sizeof(double), mb = (size_t)m * sizeof(double), ab = (size_t)d->plan->arena * sizeof(TL);
  if (ranges_overlap(d_w, nb, d_b, nb) || ranges_overlap(d_w, nb, d_g, mb) || ranges_overlap(d_g, mb, d_b, nb) || ranges_overlap(d_w, nb, d_arena, ab) ||
      ranges_overlap(d_g, mb, d_arena, ab)) {
    chol_set_error("%s: b, w, g and the arena must not overlap each other", what);
    return CHOLAMD_ERR_ARG;
  }
  HIPCHK(hipSetDevice(d->dev));
  return schur_condense_t(d, d_arena, k, t0, m, d_b, d_w, d_g, st);
}
template <class TL> static int schur_expand_api(cholamd_device *d, const TL *d_arena, int k, const double *d_w, const double *d_xt, double *d_x, hipStream_t st, const char *what)
{
  int t0 = 0;
  const int m = schur_args(d, k, what, &t0);
  if (m < 0) return m;
  if (!d_arena || !d_w || !d_xt || !d_x) { chol_set_error("%s: NULL %s", what, !d_arena ? "arena" : !d_w ? "w" : !d_xt ? "xt" : "x"); return CHOLAMD_ERR_ARG; }
  const size_t nb = (size_t)d->plan->n * sizeof(double), mb = (size_t)m * sizeof(double), ab = (size_t)d->plan->arena * sizeof(TL);
  if (ranges_overlap(d_x, nb, d_w, nb) || ranges_overlap(d_x, nb, d_xt, mb) || ranges_overlap(d_x, nb, d_arena, ab)) {
    chol_set_error("%s: x must not overlap w, xt or the arena", what);
    return CHOLAMD_ERR_ARG;
  }
  HIPCHK(hipSetDevice(d->dev));
  return schur_expand_t(d, d_arena, k, t0, m, d_w, d_xt, d_x, st);
}
extern "C" int cholamd_schur_condense(cholamd_device *d, const double *d_arena, int k, const double *d_b, double *d_w, double *d_g, void *stream)
{ return schur_condense_api(d, d_arena, k, d_b, d_w, d_g, (hipStream_t)stream, "cholamd_schur_condense"); }
extern "C" int cholamd_schur_condense_f32(cholamd_device *d, const float *d_arena32, int k, const double *d_b, double *d_w, double *d_g, void *stream)
{ return schur_condense_api(d, d_arena32, k, d_b, d_w, d_g, (hipStream_t)stream, "cholamd_schur_condense_f32"); }
extern "C" int cholamd_schur_expand(cholamd_device *d, const double *d_arena, int k, const double *d_w, const double *d_xt, double *d_x, void *stream)
{ return schur_expand_api(d, d_arena, k, d_w, d_xt, d_x, (hipStream_t)stream, "cholamd_schur_expand"); }
extern "C" int cholamd_schur_expand_f32(cholamd_device *d, const float *d_arena32, int k, const double *d_w, const double *d_xt, double *d_x, void *stream)
{ return schur_expand_api(d, d_arena32, k, d_w, d_xt, d_x, (hipStream_t)stream, "cholamd_schur_expand_f32"); }

// ---- block forms (include/cholamd.h at cholamd_schur_condense_nrhs): chunks of CHOL_NRHS_W columns through the permuted row-major block ynrhs; the pack /
// unpack kernels of chol_schur.hip stand where the block solve has its permutes.  a, b, c: the call's three blocks with their rows and names
struct schur_blk { const double *p; int64_t ld; int rows; const char *name; };
static size_t blk_bytes(const schur_blk &x, int nrhs) { return ((size_t)(nrhs - 1) * (size_t)x.ld + (size_t)x.rows) * sizeof(double); }
static int schur_nrhs_args(const cholamd_device *d, const void *arena, int k, const schur_blk (&x)[3], int nrhs, const char *what, int *t0)
{ // m, or the error; *t0 < 0: nothing to do
  const int m = schur_args(d, k, what, t0);
  if (m < 0) return m;
  if (nrhs < 0) { chol_set_error("%s: nrhs = %d < 0", what, nrhs); return CHOLAMD_ERR_ARG; }
  for (const schur_blk &b : x)
    if (b.ld < (b.rows == 0 ? m : b.rows)) { chol_set_error("%s: leading dimension of %s = %lld is less than its %d rows", what, b.name, (long long)b.ld, b.rows == 0 ? m : b.rows); return CHOLAMD_ERR_ARG; }
  if (nrhs == 0) { *t0 = -1; return m; }
  if (!arena) { chol_set_error("%s: NULL arena", what); return CHOLAMD_ERR_ARG; }
  for (const schur_blk &b : x) if (!b.p) { chol_set_error("%s: NULL %s", what, b.name); return CHOLAMD_ERR_ARG; }
  return m;
}
// what both block forms do between their checks and their chunks: the device, the lists, the chunk's block, and the inverses once per call -- whatever
// keep_inverses says; it is then set for the column-by-column chunks (keep_restore in the callers)
template <class TL> static int schur_nrhs_begin(cholamd_device *d, const TL *d_arena, int k, hipStream_t st)
{
  HIPCHK(hipSetDevice(d->dev));
  int rc = schur_build(d, k);
  if (!rc) rc = d->ynrhs.ensure((size_t)d->plan->n * CHOL_NRHS_W);
  if (!rc) rc = schur_inverses(d, d_arena, k, st);
  return rc;
}
template <class TL> static int schur_condense_nrhs_api(cholamd_device *d, const TL *d_arena, int k, const double *d_B, int64_t ldb, double *d_W, int64_t ldw, double *d_G, int64_t ldg,
                                                       int nrhs, hipStream_t st, const char *what)
{
  if (!d) { chol_set_error("%s: NULL device", what); return CHOLAMD_ERR_ARG; }
  const int n = d->plan->n;
  int t0 = 0;
  schur_blk x[3] = { { d_B, ldb, n, "B" }, { d_W, ldw, n, "W" }, { d_G, ldg, 0, "G" } };
  const int m = schur_nrhs_args(d, d_arena, k, x, nrhs, what, &t0);
  if (m < 0) return m;
  if (t0 < 0) return 0;
  x[2].rows = m;
  const size_t ab = (size_t)d->plan->arena * sizeof(TL);
  for (int i = 0; i < 3; i++) {
    if (x[i].rows == 0) continue; // (m = 0: G has no element)
    bool bad = ranges_overlap(x[i].p, blk_bytes(x[i], nrhs), d_arena, ab);
    for (int j = i + 1; j < 3 && !bad; j++) bad = x[j].rows > 0 && ranges_overlap(x[i].p, blk_bytes(x[i], nrhs), x[j].p, blk_bytes(x[j], nrhs));
    if (bad) { chol_set_error("%s: B, W, G and the arena must not overlap each other", what); return CHOLAMD_ERR_ARG; }
  }
  { int rc = schur_nrhs_begin(d, d_arena, k, st); if (rc) return rc; }
  keep_restore kr(d);
  d->keep_inverses = true;
  double *Y = d->ynrhs;
  for (int c0 = 0; c0 < nrhs; c0 += CHOL_NRHS_W) {
    const int cols = std::min(CHOL_NRHS_W, nrhs - c0);
    if (!d->schur_deterministic && cols < half_nrhs_min_block<TL>()) {
      for (int j = c0; j < c0 + cols; j++) {
        int rc = schur_condense_t(d, d_arena, k, t0, m, d_B + (int64_t)j * ldb, d_W + (int64_t)j * ldw, d_G + (int64_t)j * ldg, st);
        if (rc) return rc;
      }
      continue;
    }
    HIPCHK((hipError_t)chol_nrhs_launch_permute(d_B, ldb, d->perm, Y, nullptr, 0, n, c0, cols, 0, st));
    { int rc = schur_sweep(d, d_arena, k, false, { Y, true }, st); if (rc) return rc; }
    HIPCHK((hipError_t)chol_launch_schur_unpack(Y, n, t0, c0, cols, d_W, ldw, d_G, ldg, st));
    d->schur_launches[3]++;
  }
  return 0;
}
template <class TL> static int schur_expand_nrhs_api(cholamd_device *d, const TL *d_arena, int k, const double *d_W, int64_t ldw, const double *d_XT, int64_t ldxt, double *d_X, int64_t ldx,
                                                     int nrhs, hipStream_t st, const char *what)
{
  if (!d) { chol_set_error("%s: NULL device", what); return CHOLAMD_ERR_ARG; }
  const int n = d->plan->n;
  int t0 = 0;
  schur_blk x[3] = { { d_W, ldw, n, "W" }, { d_XT, ldxt, 0, "XT" }, { d_X, ldx, n, "X" } };
  const int m = schur_nrhs_args(d, d_arena, k, x, nrhs, what, &t0);
  if (m < 0) return m;
  if (t0 < 0) return 0;
  x[1].rows = m;
  const size_t ab = (size_t)d->plan->arena * sizeof(TL), xb = blk_bytes(x[2], nrhs);
  if (ranges_overlap(d_X, xb, d_W, blk_bytes(x[0], nrhs)) || (m > 0 && ranges_overlap(d_X, xb, d_XT, blk_bytes(x[1], nrhs))) || ranges_overlap(d_X, xb, d_arena, ab)) {
    chol_set_error("%s: X must not overlap W, XT or the arena", what);
    return CHOLAMD_ERR_ARG;
  }
  { int rc = schur_nrhs_begin(d, d_arena, k, st); if (rc) return rc; }
  keep_restore kr(d);
  d->keep_inverses = true;
  double *Y = d->ynrhs;
  for (int c0 = 0; c0 < nrhs; c0 += CHOL_NRHS_W) {
    const int cols = std::min(CHOL_NRHS_W, nrhs - c0);
    if (!d->schur_deterministic && cols < half_nrhs_min_block<TL>()) {
      for (int j = c0; j < c0 + cols; j++) {
        int rc = schur_expand_t(d, d_arena, k, t0, m, d_W + (int64_t)j * ldw, d_XT + (int64_t)j * ldxt, d_X + (int64_t)j * ldx, st);
        if (rc) return rc;
      }
      continue;
    }
    HIPCHK((hipError_t)chol_launch_schur_pack(d_W, ldw, d_XT, ldxt, n, t0, c0, cols, Y, st));
    d->schur_launches[3]++;
    { int rc = schur_sweep(d, d_arena, k, true, { Y, true }, st); if (rc) return rc; }
    HIPCHK((hipError_t)chol_nrhs_launch_permute(nullptr, 0, d->perm, Y, d_X, ldx, n, c0, cols, 1, st));
  }
  return 0;
}
extern "C" int cholamd_schur_condense_nrhs(cholamd_device *d, const double *d_arena, int k, const double *d_B, int64_t ldb, double *d_W, int64_t ldw, double *d_G, int64_t ldg, int nrhs, void *stream)
{ return schur_condense_nrhs_api(d, d_arena, k, d_B, ldb, d_W, ldw, d_G, ldg, nrhs, (hipStream_t)stream, "cholamd_schur_condense_nrhs"); }
extern "C" int cholamd_schur_condense_nrhs_f32(cholamd_device *d, const float *d_arena32, int k, const double *d_B, int64_t ldb, double *d_W, int64_t ldw, double *d_G, int64_t ldg, int nrhs, void *stream)
{ return schur_condense_nrhs_api(d, d_arena32, k, d_B, ldb, d_W, ldw, d_G, ldg, nrhs, (hipStream_t)stream, "cholamd_schur_condense_nrhs_f32"); }
extern "C" int cholamd_schur_expand_nrhs(cholamd_device *d, const double *d_arena, int k, const double *d_W, int64_t ldw, const double *d_XT, int64_t ldxt, double *d_X, int64_t ldx, int nrhs, void *stream)
{ return schur_expand_nrhs_api(d, d_arena, k, d_W, ldw, d_XT, ldxt, d_X, ldx, nrhs, (hipStream_t)stream, "cholamd_schur_expand_nrhs"); }
extern "C" int cholamd_schur_expand_nrhs_f32(cholamd_device *d, const float *d_arena32, int k, const double *d_W, int64_t ldw, const double *d_XT, int64_t ldxt, double *d_X, int64_t ldx, int nrhs, void *stream)
{ return schur_expand_nrhs_api(d, d_arena32, k, d_W, ldw, d_XT, ldxt, d_X, ldx, nrhs, (hipStream_t)stream, "cholamd_schur_expand_nrhs_f32"); }
extern "C" int cholamd_device_schur_launches(const cholamd_device *d, int64_t out[4])
{
  if (!d || !out) { chol_set_error("cholamd_device_schur_launches: NULL %s", !d ? "device" : "out"); return CHOLAMD_ERR_ARG; }
  for (int i = 0; i < 4; i++) out[i] = d->schur_launches[i];
  return 0;
}
