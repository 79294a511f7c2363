// C ABI glue of libcholamd, sparse solves: right-hand sides on a few dofs, solutions on a few dofs (include/cholamd.h at "sparse solves"; DESIGN.md section
// 19).  Compiled with hipcc like chol_api.cpp; what they share is in chol_device.h.
#include "chol_device.h"

// ---------------------------------------------------------------------------------------------
// The handle owns the PRUNED step lists of its dof lists on the device (chol_build_sparse_det: items and sources per direction, the descriptors of the
// active separators per level), the active rows of the permuted block with the input row each one takes, and the outputs' positions.  It borrows the
// device object's block ynrhs and its workspace of 16x16 inverses ws_solve; both are allocated at create, so a warm solve only enqueues.
// ---------------------------------------------------------------------------------------------
struct cholamd_sparse {
  cholamd_device *d = nullptr;
  int n_in = 0, n_out = 0, levels = 0;
  int64_t n_pos = 0, counts[12] = { 0 };
  sdet_dev lists;
  dev_buf<chol_trsv_desc> trsv[3];          // [direction], [2]: the union (the inverses of a whole solve)
  std::vector<int> lvl_first[3], lvl_max_n[3];
  dev_buf<int> act_pos, act_in, pos_out;
};
static int sparse_rank_ok(const cholamd_device *d, const char *what)
{
  if (d->world > 1 && d->rank != 0) {
    chol_set_error("%s: rank %d of %d holds its own subtrees only; the call needs the complete factor (a single-GPU object, or rank 0 after a gather)", what, d->rank, d->world);
    return CHOLAMD_ERR_ARG;
  }
  return 0;
}
extern "C" int cholamd_sparse_create(cholamd_device *d, const int *in_dofs, int n_in, const int *out_dofs, int n_out, cholamd_sparse **out)
{
  const char *what = "cholamd_sparse_create";
  if (out) *out = nullptr;
  if (!d || !out) { chol_set_error("%s: NULL %s", what, !d ? "device" : "out"); return CHOLAMD_ERR_ARG; }
  { int rc = sparse_rank_ok(d, what); if (rc) return rc; }
  const cholamd_plan *p = d->plan;
  const int n = p->n, ns = p->nsep;
  std::vector<unsigned char> act_fw((size_t)ns + 1), act_bw((size_t)ns + 1);
  std::vector<int> pos_in((size_t)std::max(n_in, 1)), pos_out((size_t)std::max(n_out, 1));
  { int rc = chol_sparse_masks(p, what, in_dofs, n_in, out_dofs, n_out, act_fw.data(), act_bw.data(), pos_in.data(), pos_out.data()); if (rc) return rc; }
  HIPCHK(hipSetDevice(d->dev));
  chol_sparse_lists w;
  { int rc = chol_build_sparse_det(p, act_fw.data(), act_bw.data(), &w); if (rc) return rc; }
  cholamd_sparse *s = new cholamd_sparse;
  s->d = d; s->n_in = n_in; s->n_out = n_out; s->levels = p->levels; s->n_pos = w.n_pos;
  chol_sparse_counts(p, &w, s->counts);
  // the active rows, ascending, and the input row each one takes (-1: it starts from zero)
  std::vector<int> act_pos, act_in, row_of((size_t)std::max(n, 1), -1);
  act_pos.reserve((size_t)w.n_pos);
  for (int r = 0; r < w.n_range; r++)
    for (int i = 0; i < w.range[2 * r + 1]; i++) { row_of[(size_t)w.range[2 * r] + i] = (int)act_pos.size(); act_pos.push_back(w.range[2 * r] + i); }
  act_in.assign(act_pos.size(), -1);
  int rc = 0;
  for (int i = 0; i < n_in && !rc; i++) {
    if (row_of[(size_t)pos_in[i]] < 0) { chol_set_error("internal: %s: input dof %d lies outside the active ranges", what, in_dofs[i]); rc = CHOLAMD_ERR_INVARIANT; }
    else act_in[(size_t)row_of[(size_t)pos_in[i]]] = i;
  }
  for (int i = 0; i < n_out && !rc; i++)
    if (row_of[(size_t)pos_out[i]] < 0) { chol_set_error("internal: %s: output dof %d lies outside the active ranges", what, out_dofs[i]); rc = CHOLAMD_ERR_INVARIANT; }
  if (!rc) rc = upload_sdet(s->lists, w.w);
  for (int q = 0; q < 3 && !rc; q++) {
    rc = s->trsv[q].upload(w.trsv[q], (size_t)w.n_act[q]);
    s->lvl_first[q].assign(w.lvl_first[q], w.lvl_first[q] + p->levels + 1);
    s->lvl_max_n[q].assign(w.lvl_max_n[q], w.lvl_max_n[q] + p->levels + 1);
  }
  if (!rc) rc = s->act_pos.upload(act_pos.data(), act_pos.size());
  if (!rc) rc = s->act_in.upload(act_in.data(), act_in.size());
  if (!rc) rc = s->pos_out.upload(pos_out.data(), (size_t)n_out);
  if (!rc) rc = d->ynrhs.ensure((size_t)n * CHOL_NRHS_W);
  if (!rc) rc = d->ws_solve.ensure((size_t)(p->ws_doubles > 0 ? p->ws_doubles : 1));
  chol_sparse_lists_free(&w);
  if (rc) { delete s; return rc; }
  *out = s;
  return 0;
}
extern "C" void cholamd_sparse_destroy(cholamd_sparse *s) { delete s; }
extern "C" int cholamd_sparse_counts(const cholamd_sparse *s, int64_t out[12])
{
  if (!s || !out) { chol_set_error("cholamd_sparse_counts: NULL %s", !s ? "object" : "out"); return CHOLAMD_ERR_ARG; }
  std::copy(s->counts, s->counts + 12, out);
  return 0;
}
// the 16x16 inverses of the active separators of list q from THIS arena, level by level
template <class TL> static int sparse_inverses(cholamd_sparse *s, const TL *d_arena, int q, hipStream_t st)
{
  for (int lvl = 0; lvl < s->levels; lvl++) {
    const int first = s->lvl_first[q][lvl], cnt = s->lvl_first[q][lvl + 1] - first;
    if (cnt > 0) HIPCHK((hipError_t)chol_launch_solve_dinv(d_arena, s->trsv[q] + first, cnt, s->lvl_max_n[q][lvl], s->d->ws_solve, st));
  }
  return 0;
}
// one sweep of the pruned lists on the block: sweep_steps' launches, the span launch on the level's ACTIVE descriptors
template <class TL> static int sparse_sweep(cholamd_sparse *s, const TL *d_arena, int q, double *Y, hipStream_t st)
{
  const sdet_dev &c = s->lists;
  const chol_mul_item *items = c.item[q];
  for (const chol_sdet_step &t : c.step[q]) {
    if (t.item_end > t.item_first) HIPCHK((hipError_t)chol_launch_solve_det_gather_nrhs(d_arena, items + t.item_first, t.item_end - t.item_first, c.src[q], q, Y, st));
    if (t.col0 >= 0) {
      const int first = s->lvl_first[q][t.level], cnt = s->lvl_first[q][t.level + 1] - first;
      HIPCHK((hipError_t)chol_nrhs_launch_span(d_arena, s->trsv[q] + first, cnt, s->d->ws_solve, Y, t.col0, q, st));
    }
  }
  return 0;
}
template <class TL> static int sparse_solve_t(cholamd_sparse *s, const TL *d_arena, const double *d_Bs, int64_t ldb, double *d_Xs, int64_t ldx, int nrhs, int which, hipStream_t st, const char *what)
{
  if (!s) { chol_set_error("%s: NULL object", what); return CHOLAMD_ERR_ARG; }
  cholamd_device *d = s->d;
  if (which != CHOLAMD_HALF_FORWARD && which != CHOLAMD_HALF_BACKWARD && which != CHOL_BOTH_SWEEPS) {
    chol_set_error("%s: which = %d is neither CHOLAMD_HALF_FORWARD (0), CHOLAMD_HALF_BACKWARD (1) nor -1 (the whole solve)", what, which);
    return CHOLAMD_ERR_ARG;
  }
  if (nrhs < 0) { chol_set_error("%s: nrhs = %d < 0", what, nrhs); return CHOLAMD_ERR_ARG; }
  if (ldb < s->n_in || ldx < s->n_out) {
    chol_set_error("%s: leading dimensions ldb = %lld, ldx = %lld must be at least n_in = %d, n_out = %d", what, (long long)ldb, (long long)ldx, s->n_in, s->n_out);
    return CHOLAMD_ERR_ARG;
  }
  { int rc = sparse_rank_ok(d, what); if (rc) return rc; }
  if (nrhs == 0) return 0;
  if (!d_arena || !d_Bs || !d_Xs) { chol_set_error("%s: NULL %s", what, !d_arena ? "arena" : !d_Bs ? "Bs" : "Xs"); return CHOLAMD_ERR_ARG; }
  if ((const void *)d_Bs == (const void *)d_Xs && (s->n_in != s->n_out || ldb != ldx)) {
    chol_set_error("%s: Xs aliases Bs with n_in = %d, n_out = %d, ldb = %lld, ldx = %lld: in place needs n_in == n_out and ldb == ldx", what, s->n_in, s->n_out, (long long)ldb, (long long)ldx);
    return CHOLAMD_ERR_ARG;
  }
  HIPCHK(hipSetDevice(d->dev));
  double *Y = d->ynrhs;
  { int rc = sparse_inverses(s, d_arena, which == CHOL_BOTH_SWEEPS ? 2 : which, st); if (rc) return rc; }
  for (int c0 = 0; c0 < nrhs; c0 += CHOL_NRHS_W) {
    const int cols = std::min(CHOL_NRHS_W, nrhs - c0);
    HIPCHK((hipError_t)chol_launch_sparse_load(d_Bs, ldb, s->act_pos, s->act_in, s->n_pos, c0, cols, Y, st));
    for (int q = 0; q < 2; q++) {
      if (which != CHOL_BOTH_SWEEPS && which != q) continue;
      int rc = sparse_sweep(s, d_arena, q, Y, st);
      if (rc) return rc;
    }
    HIPCHK((hipError_t)chol_launch_sparse_store(Y, s->pos_out, s->n_out, d_Xs, ldx, c0, cols, st));
  }
  return 0;
}
extern "C" int cholamd_sparse_solve_nrhs(cholamd_sparse *s, const double *d_arena, const double *d_Bs, int64_t ldb, double *d_Xs, int64_t ldx, int nrhs, int which, void *stream)
{ return sparse_solve_t(s, d_arena, d_Bs, ldb, d_Xs, ldx, nrhs, which, (hipStream_t)stream, "cholamd_sparse_solve_nrhs"); }
extern "C" int cholamd_sparse_solve_nrhs_f32(cholamd_sparse *s, const float *d_arena32, const double *d_Bs, int64_t ldb, double *d_Xs, int64_t ldx, int nrhs, int which, void *stream)
{ return sparse_solve_t(s, d_arena32, d_Bs, ldb, d_Xs, ldx, nrhs, which, (hipStream_t)stream, "cholamd_sparse_solve_nrhs_f32"); }
