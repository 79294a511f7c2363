// C ABI glue of libcholamd, what is read off a finished factor: its diagonal and determinant, selected inversion, the gradients with respect to A's
// values and the forward products.  Compiled with hipcc like chol_api.cpp; what they share is in chol_device.h.
#include "chol_device.h"

// ---------------------------------------------------------------------------------------------
// The factor's diagonal and determinant (include/cholamd.h at cholamd_factor_diag)
// ---------------------------------------------------------------------------------------------
template <class TL> static int factor_diag_t(cholamd_device *d, const TL *d_arena, double *d_diag, hipStream_t st, const char *what)
{
  if (!d) { chol_set_error("%s: NULL device", what); return CHOLAMD_ERR_ARG; }
  if (!d_arena || !d_diag) { chol_set_error("%s: NULL %s", what, !d_arena ? "arena" : "d_diag"); return CHOLAMD_ERR_ARG; }
  HIPCHK(hipSetDevice(d->dev));
  { int rc = build_solve(d); if (rc) return rc; }
  HIPCHK((hipError_t)chol_launch_factor_diag(d_arena, d->dg_desc, d->dg_prefix, d->n_dg, d->plan->n, d->perm, d_diag, st));
  return 0;
}
template <class TL> static int factor_logdet_t(cholamd_device *d, const TL *d_arena, double *logdet_out, hipStream_t st, const char *what)
{
  if (logdet_out) *logdet_out = std::nan("");
  if (!d) { chol_set_error("%s: NULL device", what); return CHOLAMD_ERR_ARG; }
  if (!d_arena || !logdet_out) { chol_set_error("%s: NULL %s", what, !d_arena ? "arena" : "logdet_out"); return CHOLAMD_ERR_ARG; }
  HIPCHK(hipSetDevice(d->dev));
  { int rc = build_solve(d); if (rc) return rc; }
  int rc = d->ld_part.ensure(2 * CHOL_LOGDET_MAX_BLOCKS);
  if (!rc) rc = d->ld_ipart.ensure(2 * CHOL_LOGDET_MAX_BLOCKS);
  if (!rc) rc = d->ld_res.ensure(3);
  if (rc) return rc;
  HIPCHK((hipError_t)chol_launch_factor_logdet(d_arena, d->dg_desc, d->dg_prefix, d->n_dg, d->plan->n, d->ld_part, d->ld_ipart, d->ld_res, st));
  int64_t res[3] = { 0, 0, 0 };
  HIPCHK(hipMemcpyAsync(res, d->ld_res, sizeof res, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (res[1] > 0) {
    const cholamd_plan *p = d->plan;
    const int pos = (int)res[2], sep = p->sep_of_pos[pos];
    chol_set_error("%s: %lld of the factor's diagonal entries %s not positive and finite, the first in column %d of separator %d (permuted position %d): "
                   "the arena holds no valid factor", what, (long long)res[1], res[1] == 1 ? "is" : "are", pos - p->sep_off[sep] + 1, sep, pos);
    return CHOLAMD_ERR_ARG;
  }
  std::memcpy(logdet_out, &res[0], sizeof(double));
  return 0;
}
extern "C" int cholamd_factor_diag(cholamd_device *d, const double *d_arena, double *d_diag, void *stream) { return factor_diag_t(d, d_arena, d_diag, (hipStream_t)stream, "cholamd_factor_diag"); }
extern "C" int cholamd_factor_diag_f32(cholamd_device *d, const float *d_arena32, double *d_diag, void *stream) { return factor_diag_t(d, d_arena32, d_diag, (hipStream_t)stream, "cholamd_factor_diag_f32"); }
extern "C" int cholamd_factor_logdet(cholamd_device *d, const double *d_arena, double *logdet_out, void *stream) { return factor_logdet_t(d, d_arena, logdet_out, (hipStream_t)stream, "cholamd_factor_logdet"); }
extern "C" int cholamd_factor_logdet_f32(cholamd_device *d, const float *d_arena32, double *logdet_out, void *stream) { return factor_logdet_t(d, d_arena32, logdet_out, (hipStream_t)stream, "cholamd_factor_logdet_f32"); }

// ---------------------------------------------------------------------------------------------
// Selected inversion (include/cholamd.h at cholamd_selinv; kernels and launch structure in chol_selinv.hip).  The gather lists depend on the plan alone:
// they are built at the first call on a device object, beside the solve lists, and stay until it is destroyed -- device creation and the factor path do
// not pay for them.
// ---------------------------------------------------------------------------------------------
static int build_selinv(cholamd_device *d)
{
  if (d->si_ready) return 0;
  const int L = d->plan->levels;
  std::vector<selinv_dev> si(L); // handed to the device object once complete
  int64_t ws = 1;
  for (int lvl = 0; lvl < L; lvl++) {
    chol_selinv_level w;
    int rc = chol_build_selinv_level(d->plan, lvl, &w);
    if (rc) return rc;
    selinv_dev &s = si[lvl];
    s.host.assign(w.sep, w.sep + w.n_sep);
    s.max_nblk = w.max_nblk;
    if (w.max_tiles > CHOL_SELINV_MAX_TILES) {
      chol_set_error("cholamd_selinv: a panel of level %d stores %d 16-row tiles, the step launches take %d", lvl, w.max_tiles, CHOL_SELINV_MAX_TILES);
      chol_selinv_level_free(&w);
      return CHOLAMD_ERR_ARG;
    }
    ws = std::max(ws, w.ws_doubles);
    rc = s.sep.upload(w.sep, (size_t)w.n_sep);
    if (!rc) rc = s.tile.upload(w.tile, (size_t)w.n_tile);
    if (!rc) rc = s.chain_ld.upload(w.chain_ld, (size_t)w.n_chain);
    if (!rc) rc = s.chain_pos0.upload(w.chain_pos0, (size_t)w.n_chain);
    if (!rc) rc = s.rowoff.upload(w.rowoff, (size_t)w.n_rowoff);
    chol_selinv_level_free(&w);
    if (rc) return rc;
  }
  { int rc = d->si_ws.alloc((size_t)ws); if (rc) return rc; }
  d->si = std::move(si);
  d->si_ready = true;
  return 0;
}
extern "C" int cholamd_selinv(cholamd_device *d, const double *d_arena, double *d_zarena, void *stream)
{
  if (!d) { chol_set_error("cholamd_selinv: NULL device"); return CHOLAMD_ERR_ARG; }
  if (!d_arena || !d_zarena) { chol_set_error("cholamd_selinv: NULL %s", !d_arena ? "arena" : "Z arena"); return CHOLAMD_ERR_ARG; }
  const int64_t na = d->plan->arena;
  if (d_zarena < d_arena + na && d_arena < d_zarena + na) {
    chol_set_error("cholamd_selinv: the Z arena overlaps the factor's arena (there is no in-place form)");
    return CHOLAMD_ERR_ARG;
  }
  if (d->world > 1 && d->rank != 0) {
    chol_set_error("cholamd_selinv: rank %d of %d holds its own subtrees only; the call needs the complete factor (a single-GPU object, or rank 0 after a gather)", d->rank, d->world);
    return CHOLAMD_ERR_ARG;
  }
  HIPCHK(hipSetDevice(d->dev));
  { int rc = build_selinv(d); if (rc) return rc; }
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(d_zarena, 0, (size_t)na * sizeof(double), st)); // padding rows, the upper triangles of the diagonal blocks: every stored position is defined
  for (int lvl = 0; lvl < d->plan->levels; lvl++) { // root first: a separator gathers from its ancestors' finished panels
    const selinv_dev &s = d->si[lvl];
    for (int step = 0; step < s.max_nblk; step++) {
      int n_act = 0, below = 0; // the separators with a block left are a prefix of the list
      for (const chol_selinv_sep &q : s.host) {
        if (q.nblk <= step) break;
        const int j1 = std::min((q.nblk - step) * CHOL_SELINV_W, q.w);
        below = std::max(below, q.ntile - (j1 == q.w ? q.nown : j1 / CHOL_NB));
        n_act++;
      }
      HIPCHK((hipError_t)chol_launch_selinv_step(d_arena, d_zarena, d->si_ws, s.sep, n_act, s.tile, s.chain_ld, s.chain_pos0, s.rowoff, step, below, st));
    }
  }
  return 0;
}
// k_factor_diag on the Z arena: the walk over the diagonal is the factor's
extern "C" int cholamd_selinv_diag(cholamd_device *d, const double *d_zarena, double *d_diag, void *stream) { return factor_diag_t(d, d_zarena, d_diag, (hipStream_t)stream, "cholamd_selinv_diag"); }
extern "C" int cholamd_selinv_entries(cholamd_device *d, const double *d_zarena, double *d_vals, int64_t count, void *stream)
{
  if (!d) { chol_set_error("cholamd_selinv_entries: NULL device"); return CHOLAMD_ERR_ARG; }
  if (!d_zarena || !d_vals) { chol_set_error("cholamd_selinv_entries: NULL %s", !d_zarena ? "Z arena" : "d_vals"); return CHOLAMD_ERR_ARG; }
  const cholamd_plan *p = d->plan;
  if (count != p->nz_file) { chol_set_error("cholamd_selinv_entries: room for %lld entries, the plan has %d", (long long)count, p->nz_file); return CHOLAMD_ERR_ARG; }
  HIPCHK(hipSetDevice(d->dev));
  if (!d->a_src) { int rc = d->a_src.upload(p->a_src, (size_t)p->nnz_a); if (rc) return rc; } // the index list of cholamd_device_set_values
  HIPCHK((hipError_t)chol_launch_selinv_entries(d_zarena, d->a_dst, d->a_src, p->nnz_a, d_vals, count, (hipStream_t)stream));
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Gradients with respect to the value array (include/cholamd.h at cholamd_values_grad_pairs; kernels in chol_values_grad.hip, host restatements in
// chol_symbolic.c).  The entry list and the entries' classes go to the device at the first call on a device object; later calls allocate nothing.
// ---------------------------------------------------------------------------------------------
// the rules both calls share: the plan's (count, dropped, duplicates) and the single-GPU object; then the lists
static int values_grad_ready(cholamd_device *d, int64_t count, const char *what)
{
  const cholamd_plan *p = d->plan;
  { int rc = chol_values_grad_plan_ok(p, count, what); if (rc) return rc; }
  if (d->world > 1) {
    chol_set_error("%s: the device object is rank %d of a partition of %d; gradients are taken on a single-GPU object", what, d->rank, d->world);
    return CHOLAMD_ERR_ARG;
  }
  return 0;
}
static int values_grad_lists(cholamd_device *d)
{
  const cholamd_plan *p = d->plan;
  int rc = 0;
  if (!d->e_row) rc = d->e_row.upload(p->e_row, (size_t)p->nz_file);
  if (!rc && !d->e_col) rc = d->e_col.upload(p->e_col, (size_t)p->nz_file);
  if (!rc && !d->e_cls) rc = d->e_cls.upload(p->e_cls, (size_t)p->nz_file); // (cholamd_device_set_values may have brought it)
  if (!rc && !d->a_src) rc = d->a_src.upload(p->a_src, (size_t)p->nnz_a);
  return rc;
}
extern "C" int cholamd_values_grad_pairs(cholamd_device *d, const double *d_P, int64_t ldp, const double *d_Q, int64_t ldq, int nrhs, double alpha, double beta,
                                         double *d_g, int64_t count, void *stream)
{
  const char *what = "cholamd_values_grad_pairs";
  if (!d) { chol_set_error("%s: NULL device", what); return CHOLAMD_ERR_ARG; }
  { int rc = values_grad_ready(d, count, what); if (rc) return rc; }
  const cholamd_plan *p = d->plan;
  const int n = p->n;
  if (nrhs < 0) { chol_set_error("%s: nrhs = %d < 0", what, nrhs); return CHOLAMD_ERR_ARG; }
  if (ldp < n || ldq < n) { chol_set_error("%s: leading dimensions ldp = %lld, ldq = %lld must be at least n = %d", what, (long long)ldp, (long long)ldq, n); return CHOLAMD_ERR_ARG; }
  if (nrhs == 0) return 0;
  if (!d_P || !d_Q || !d_g) { chol_set_error("%s: NULL %s", what, !d_P ? "P" : !d_Q ? "Q" : "g"); return CHOLAMD_ERR_ARG; }
  const size_t gb = (size_t)count * sizeof(double);
  const size_t pb = ((size_t)(nrhs - 1) * (size_t)ldp + (size_t)n) * sizeof(double), qb = ((size_t)(nrhs - 1) * (size_t)ldq + (size_t)n) * sizeof(double);
  if (ranges_overlap(d_g, gb, d_P, pb) || ranges_overlap(d_g, gb, d_Q, qb)) { chol_set_error("%s: g overlaps P or Q", what); return CHOLAMD_ERR_ARG; }
  HIPCHK(hipSetDevice(d->dev));
  { int rc = values_grad_lists(d); if (rc) return rc; }
  HIPCHK((hipError_t)chol_launch_values_grad_pairs(d_P, ldp, d_Q, ldq, nrhs, d->e_row, d->e_col, d->e_cls, count, alpha, beta, d_g, (hipStream_t)stream));
  return 0;
}
extern "C" int cholamd_values_grad_logdet(cholamd_device *d, const double *d_zarena, double alpha, double beta, double *d_g, int64_t count, void *stream)
{
  const char *what = "cholamd_values_grad_logdet";
  if (!d) { chol_set_error("%s: NULL device", what); return CHOLAMD_ERR_ARG; }
  { int rc = values_grad_ready(d, count, what); if (rc) return rc; }
  if (!d_zarena || !d_g) { chol_set_error("%s: NULL %s", what, !d_zarena ? "Z arena" : "g"); return CHOLAMD_ERR_ARG; }
  const cholamd_plan *p = d->plan;
  if (ranges_overlap(d_g, (size_t)count * sizeof(double), d_zarena, (size_t)p->arena * sizeof(double))) { chol_set_error("%s: g overlaps the Z arena", what); return CHOLAMD_ERR_ARG; }
  HIPCHK(hipSetDevice(d->dev));
  { int rc = values_grad_lists(d); if (rc) return rc; }
  HIPCHK((hipError_t)chol_launch_values_grad_logdet(d_zarena, d->a_dst, d->a_src, p->nnz_a, d->e_row, d->e_col, d->e_cls, count, alpha, beta, d_g, (hipStream_t)stream));
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Forward products with the factor (include/cholamd.h at cholamd_multiply_half; kernels in chol_multiply.hip): y = M z, M^T z, M M^T z with M = P^T L P.
// The owner lists depend on the plan alone: built and uploaded at the first call on a device object, kept until it is destroyed.  A half product is the
// permute of z into the work vector and ONE launch over the whole tree, which writes y in original dof order; the full product puts the BACKWARD launch
// between them, into the object's second vector (permuted coordinates throughout).
// ---------------------------------------------------------------------------------------------
static int build_multiply(cholamd_device *d)
{
  if (d->mul_ready) return 0;
  chol_mul_lists w;
  int rc = chol_build_multiply(d->plan, &w);
  if (rc) return rc;
  for (int q = 0; q < 2 && !rc; q++) { // (an upload replaces what a call that failed half-way left)
    rc = d->mul_item[q].upload(w.item[q], (size_t)w.n_item[q]);
    if (!rc) rc = d->mul_src[q].upload(w.src[q], (size_t)w.n_src[q]);
    d->n_mul_item[q] = w.n_item[q];
  }
  chol_mul_lists_free(&w);
  const size_t n = (size_t)(d->plan->n > 0 ? d->plan->n : 1);
  if (!rc) rc = d->ytmp.ensure(n);
  if (!rc) rc = d->mvec.ensure(n);
  if (rc) return rc;
  d->mul_ready = true;
  return 0;
}
// the checks every product shares, after the NULL / which / nrhs rules of the half solves: the complete factor, y outside the arena
template <class TL> static int multiply_check(cholamd_device *d, const TL *d_arena, const double *d_y, int64_t y_doubles, const char *what)
{
  if (d->world > 1 && d->rank != 0) {
    chol_set_error("%s: rank %d of %d holds its own subtrees only; the call needs the complete factor (a single-GPU object, or rank 0 after a gather)", what, d->rank, d->world);
    return CHOLAMD_ERR_ARG;
  }
  if (d_y && ranges_overlap(d_arena, (size_t)d->plan->arena * sizeof(TL), d_y, (size_t)y_doubles * sizeof(double))) {
    chol_set_error("%s: the result overlaps the factor's arena", what);
    return CHOLAMD_ERR_ARG;
  }
  return 0;
}
// which: one CHOLAMD_HALF_* product, or CHOL_BOTH_SWEEPS: y = M M^T z (BACKWARD, then FORWARD)
template <class TL> static int multiply_t(cholamd_device *d, const TL *d_arena, const double *d_z, double *d_y, int which, hipStream_t st)
{
  { int rc = build_multiply(d); if (rc) return rc; }
  const int n = d->plan->n, F = CHOLAMD_HALF_FORWARD, B = CHOLAMD_HALF_BACKWARD;
  HIPCHK((hipError_t)chol_launch_permute(d_z, d->perm, d->ytmp, n, 0, st)); // (first: d_y may be d_z)
  const double *in = d->ytmp;
  if (which == CHOL_BOTH_SWEEPS) {
    HIPCHK((hipError_t)chol_launch_multiply(d_arena, d->mul_item[B], d->n_mul_item[B], d->mul_src[B], 1, in, d->mvec, nullptr, st));
    in = d->mvec;
    which = F;
  }
  HIPCHK((hipError_t)chol_launch_multiply(d_arena, d->mul_item[which], d->n_mul_item[which], d->mul_src[which], which == B, in, d_y, d->perm, st));
  return 0;
}
template <class TL> static int multiply_half_api(cholamd_device *d, const TL *d_arena, const double *d_z, double *d_y, bool half, int which, hipStream_t st, const char *what)
{
  if (!d) { chol_set_error("%s: NULL device", what); return CHOLAMD_ERR_ARG; }
  if (half) { int rc = half_which_ok(which, what); if (rc) return rc; } // (a caller's which = -1 must not be taken for the full product)
  else which = CHOL_BOTH_SWEEPS;
  if (!d_arena || !d_z || !d_y) { chol_set_error("%s: NULL %s", what, !d_arena ? "arena" : !d_z ? "z" : "y"); return CHOLAMD_ERR_ARG; }
  { int rc = multiply_check(d, d_arena, d_y, d->plan->n, what); if (rc) return rc; }
  HIPCHK(hipSetDevice(d->dev));
  return multiply_t(d, d_arena, d_z, d_y, which, st);
}
extern "C" int cholamd_multiply_half(cholamd_device *d, const double *d_arena, const double *d_z, double *d_y, int which, void *stream)
{ return multiply_half_api(d, d_arena, d_z, d_y, true, which, (hipStream_t)stream, "cholamd_multiply_half"); }
extern "C" int cholamd_multiply_half_f32(cholamd_device *d, const float *d_arena32, const double *d_z, double *d_y, int which, void *stream)
{ return multiply_half_api(d, d_arena32, d_z, d_y, true, which, (hipStream_t)stream, "cholamd_multiply_half_f32"); }
extern "C" int cholamd_multiply(cholamd_device *d, const double *d_arena, const double *d_z, double *d_y, void *stream)
{ return multiply_half_api(d, d_arena, d_z, d_y, false, 0, (hipStream_t)stream, "cholamd_multiply"); }
extern "C" int cholamd_multiply_f32(cholamd_device *d, const float *d_arena32, const double *d_z, double *d_y, void *stream)
{ return multiply_half_api(d, d_arena32, d_z, d_y, false, 0, (hipStream_t)stream, "cholamd_multiply_f32"); }
// ---------------------------------------------------------------------------------------------
// Block form of the products (include/cholamd.h at cholamd_multiply_half_nrhs; kernel in chol_multiply_nrhs.hip): the columns in chunks of CHOL_NRHS_W = 32.
// A chunk is permuted into the object's first block, then ONE launch per direction over the items of the single-vector products; the last launch writes
// Y in original dof order itself.  The full product puts the BACKWARD launch between them, into the second block.
// ---------------------------------------------------------------------------------------------
// A block chunk costs nearly the same for 1 and for 32 columns (one pass over the factor), so a chunk of fewer columns than this goes column by column
// through the single-vector products.  min = ceil(T_chunk(32 columns) / T_single) from the medians measured on one MI355X at gen:60:8, both in one process
// (DESIGN.md section 13, table "Block form: measured times"): fp64 factor 1.035 / 0.603 ms FORWARD, 1.323 / 0.550 BACKWARD, 2.269 / 1.142 full; fp32
// factor 0.905 / 0.971, 1.188 / 0.554, 2.002 / 1.516.
template <class TL> static constexpr int multiply_nrhs_min_block(int which)
{
  return sizeof(TL) == sizeof(double) ? (which == CHOLAMD_HALF_FORWARD ? 2 : which == CHOLAMD_HALF_BACKWARD ? 3 : 2)
                                      : (which == CHOLAMD_HALF_FORWARD ? 1 : which == CHOLAMD_HALF_BACKWARD ? 3 : 2);
}
template <class TL> static int multiply_nrhs_t(cholamd_device *d, const TL *d_arena, const double *d_Z, int64_t ldz, double *d_Y, int64_t ldy, int nrhs, int which, hipStream_t st)
{
  { int rc = build_multiply(d); if (rc) return rc; }
  const int n = d->plan->n, F = CHOLAMD_HALF_FORWARD, B = CHOLAMD_HALF_BACKWARD;
  const int min_block = d->multiply_nrhs_min > 0 ? d->multiply_nrhs_min : multiply_nrhs_min_block<TL>(which);
  for (int c0 = 0; c0 < nrhs; c0 += CHOL_NRHS_W) {
    const int cols = std::min(CHOL_NRHS_W, nrhs - c0);
    if (cols < min_block) {
      for (int j = c0; j < c0 + cols; j++) { int rc = multiply_t(d, d_arena, d_Z + (int64_t)j * ldz, d_Y + (int64_t)j * ldy, which, st); if (rc) return rc; }
      continue;
    }
    const size_t blk = (size_t)(n > 0 ? n : 1) * CHOL_NRHS_W;
    { int rc = d->mznrhs.ensure(blk); if (!rc) rc = d->mwnrhs.ensure(blk); if (rc) return rc; }
    HIPCHK((hipError_t)chol_nrhs_launch_permute(d_Z, ldz, d->perm, d->mznrhs, nullptr, 0, n, c0, cols, 0, st)); // (first: Y may be Z)
    const double *in = d->mznrhs;
    int last = which;
    if (which == CHOL_BOTH_SWEEPS) {
      HIPCHK((hipError_t)chol_launch_multiply_nrhs(d_arena, d->mul_item[B], d->n_mul_item[B], d->mul_src[B], 1, in, d->mwnrhs, nullptr, 0, 0, CHOL_NRHS_W, st));
      in = d->mwnrhs;
      last = F;
    }
    HIPCHK((hipError_t)chol_launch_multiply_nrhs(d_arena, d->mul_item[last], d->n_mul_item[last], d->mul_src[last], last == B, in, d_Y, d->perm, ldy, c0, cols, st));
  }
  return 0;
}
template <class TL> static int multiply_nrhs_api(cholamd_device *d, const TL *d_arena, const double *d_Z, int64_t ldz, double *d_Y, int64_t ldy, int nrhs, bool half, int which, hipStream_t st, const char *what)
{
  if (d && half) { int rc = half_which_ok(which, what); if (rc) return rc; }
  if (!half) which = CHOL_BOTH_SWEEPS;
  { int rc = nrhs_check(d, d_arena, d_Z, ldz, d_Y, ldy, nrhs, what, "Z", "Y"); if (rc) return rc > 0 ? 0 : rc; }
  { int rc = multiply_check(d, d_arena, d_Y, (int64_t)(nrhs - 1) * ldy + d->plan->n, what); if (rc) return rc; }
  HIPCHK(hipSetDevice(d->dev));
  return multiply_nrhs_t(d, d_arena, d_Z, ldz, d_Y, ldy, nrhs, which, st);
}
extern "C" int cholamd_multiply_half_nrhs(cholamd_device *d, const double *d_arena, const double *d_Z, int64_t ldz, double *d_Y, int64_t ldy, int nrhs, int which, void *stream)
{ return multiply_nrhs_api(d, d_arena, d_Z, ldz, d_Y, ldy, nrhs, true, which, (hipStream_t)stream, "cholamd_multiply_half_nrhs"); }
extern "C" int cholamd_multiply_half_nrhs_f32(cholamd_device *d, const float *d_arena32, const double *d_Z, int64_t ldz, double *d_Y, int64_t ldy, int nrhs, int which, void *stream)
{ return multiply_nrhs_api(d, d_arena32, d_Z, ldz, d_Y, ldy, nrhs, true, which, (hipStream_t)stream, "cholamd_multiply_half_nrhs_f32"); }
extern "C" int cholamd_multiply_nrhs(cholamd_device *d, const double *d_arena, const double *d_Z, int64_t ldz, double *d_Y, int64_t ldy, int nrhs, void *stream)
{ return multiply_nrhs_api(d, d_arena, d_Z, ldz, d_Y, ldy, nrhs, false, 0, (hipStream_t)stream, "cholamd_multiply_nrhs"); }
extern "C" int cholamd_multiply_nrhs_f32(cholamd_device *d, const float *d_arena32, const double *d_Z, int64_t ldz, double *d_Y, int64_t ldy, int nrhs, void *stream)
{ return multiply_nrhs_api(d, d_arena32, d_Z, ldz, d_Y, ldy, nrhs, false, 0, (hipStream_t)stream, "cholamd_multiply_nrhs_f32"); }
template <class TL> static int factor_residual_t(cholamd_device *d, const TL *d_arena, const double *d_z, double *rel_out, hipStream_t st, const char *what)
{
  if (rel_out) *rel_out = std::nan("");
  if (!d) { chol_set_error("%s: NULL device", what); return CHOLAMD_ERR_ARG; }
  if (!d_arena || !d_z || !rel_out) { chol_set_error("%s: NULL %s", what, !d_arena ? "arena" : !d_z ? "z" : "rel_out"); return CHOLAMD_ERR_ARG; }
  { int rc = multiply_check(d, d_arena, (const double *)nullptr, 0, what); if (rc) return rc; }
  HIPCHK(hipSetDevice(d->dev));
  { int rc = ensure_refine(d); if (rc) return rc; } // the residual operator with the CURRENT values (cholamd_device_set_values keeps it up to date)
  const int n = d->plan->n, nb = (n + 255) / 256;
  int rc = d->mr_part.ensure((size_t)2 * (nb > 0 ? nb : 1));
  if (!rc) rc = d->mr_ipart.ensure((size_t)(nb > 0 ? nb : 1));
  if (!rc) rc = d->mr_res.ensure(3);
  if (rc) return rc;
  if ((rc = multiply_t(d, d_arena, d_z, d->rvec, CHOL_BOTH_SWEEPS, st))) return rc; // w = M M^T z in original dof order
  HIPCHK((hipError_t)chol_launch_multiply_resid(d->csr_ptr, d->csr_col, d->csr_val, d_z, d->rvec, n, d->mr_part, d->mr_ipart, d->mr_res, st));
  int64_t res[3] = { 0, 0, 0 };
  HIPCHK(hipMemcpyAsync(res, d->mr_res, sizeof res, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  double d2, a2;
  std::memcpy(&d2, &res[0], sizeof d2); std::memcpy(&a2, &res[1], sizeof a2);
  if (res[2] > 0 || !(d2 <= DBL_MAX) || !(a2 <= DBL_MAX)) {
    chol_set_error("%s: A z or M M^T z is not finite in %lld rows (a NaN or inf in z, in the values of A or in the arena)", what, (long long)res[2]);
    return CHOLAMD_ERR_ARG;
  }
  *rel_out = a2 > 0.0 ? std::sqrt(d2 / a2) : std::sqrt(d2);
  return 0;
}
extern "C" int cholamd_factor_residual(cholamd_device *d, const double *d_arena, const double *d_z, double *rel_out, void *stream)
{ return factor_residual_t(d, d_arena, d_z, rel_out, (hipStream_t)stream, "cholamd_factor_residual"); }
extern "C" int cholamd_factor_residual_f32(cholamd_device *d, const float *d_arena32, const double *d_z, double *rel_out, void *stream)
{ return factor_residual_t(d, d_arena32, d_z, rel_out, (hipStream_t)stream, "cholamd_factor_residual_f32"); }
