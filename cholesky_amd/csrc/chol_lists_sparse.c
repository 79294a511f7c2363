/* Sparse solves (cholamd_sparse_*; include/cholamd.h at "sparse solves"): right-hand sides that are non-zero on a few dofs, solutions
 * wanted on a few dofs.  The step lists of the deterministic solve (chol_build_solve_det) PRUNED to the separators that hold those dofs and their ancestors,
 * with their host restatement.  No second solve path: the pruned lists have the format of the full ones and go through the same kernels. */
#define _GNU_SOURCE
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "chol_plan.h"
#include "cholamd.h"

void chol_sparse_lists_free(chol_sparse_lists *w)
{
  chol_sdet_lists_free(&w->w);
  for (int q = 0; q < 3; q++) { free(w->trsv[q]); free(w->lvl_first[q]); free(w->lvl_max_n[q]); }
  free(w->range);
  memset(w, 0, sizeof *w);
}

int chol_sparse_masks(const plan_t *p, const char *what, const int *in_dofs, int n_in, const int *out_dofs, int n_out, unsigned char *act_fw, unsigned char *act_bw,
                      int *pos_in, int *pos_out)
{
  if (!in_dofs || !out_dofs) { chol_set_error("%s: NULL %s", what, !in_dofs ? "in_dofs" : "out_dofs"); return CHOLAMD_ERR_ARG; }
  if (n_in < 1 || n_out < 1) { chol_set_error("%s: %s = %d < 1", what, n_in < 1 ? "n_in" : "n_out", n_in < 1 ? n_in : n_out); return CHOLAMD_ERR_ARG; }
  const int n = p->n, ns = p->nsep;
  unsigned char *seen = calloc((size_t)(n > 0 ? n : 1), 1);
  if (!seen) { chol_set_error("out of memory"); return CHOLAMD_ERR_NOMEM; }
  for (int side = 0; side < 2; side++) {
    const int *dofs = side ? out_dofs : in_dofs, cnt = side ? n_out : n_in;
    unsigned char *act = side ? act_bw : act_fw;
    int *pos = side ? pos_out : pos_in;
    memset(act, 0, (size_t)ns + 1);
    for (int i = 0; i < cnt; i++) {
      const int dof = dofs[i];
      if (dof < 0 || dof >= n) { chol_set_error("%s: %s[%d] = %d is not a dof in [0, %d)", what, side ? "out_dofs" : "in_dofs", i, dof, n); free(seen); return CHOLAMD_ERR_ARG; }
      if (seen[dof] & (1 << side)) { chol_set_error("%s: %s[%d] = %d is a duplicate", what, side ? "out_dofs" : "in_dofs", i, dof); free(seen); return CHOLAMD_ERR_ARG; }
      seen[dof] |= (unsigned char)(1 << side);
      if (pos) pos[i] = p->iperm[dof];
      for (int h = p->heap_of[p->sep_of_pos[p->iperm[dof]]]; h >= 1 && !act[p->tree[h]]; h >>= 1) act[p->tree[h]] = 1; /* up to the first marked ancestor: its own are marked */
    }
  }
  free(seen);
  return 0;
}

int chol_build_sparse_det(const plan_t *p, const unsigned char *act_fw, const unsigned char *act_bw, chol_sparse_lists *out)
{
  memset(out, 0, sizeof *out);
  const int ns = p->nsep, L = p->levels, n = p->n, SP = CHOL_SDET_SPAN;
  const unsigned char *act[2] = { act_fw, act_bw };
  for (int q = 0; q < 2; q++)
    for (int h = 2; h <= ns; h++)
      if (act[q][p->tree[h]] && !act[q][p->tree[h >> 1]]) { chol_set_error("internal: sparse solve: the active set of direction %d holds separator %d but not its parent %d", q, p->tree[h], p->tree[h >> 1]); return CHOLAMD_ERR_INVARIANT; }
  chol_sdet_lists w;
  int rc = chol_build_solve_det(p, &w);
  if (rc) return rc;
  unsigned char *solved = calloc((size_t)(n > 0 ? n : 1), 1);
  int *stamp = malloc((size_t)(n > 0 ? n : 1) * sizeof(int)), *lvl_wide[2] = { calloc((size_t)L + 1, sizeof(int)), calloc((size_t)L + 1, sizeof(int)) };
  rc = CHOLAMD_ERR_NOMEM;
  if (!solved || !stamp || !lvl_wide[0] || !lvl_wide[1]) { chol_set_error("out of memory"); goto done; }
  /* the descriptors of the active separators, level by level in the order of the level's own list; lvl_wide[q][l] = the widest active one of the direction */
  for (int q = 0; q < 3; q++) {
    out->trsv[q] = calloc((size_t)ns + 1, sizeof(chol_trsv_desc));
    out->lvl_first[q] = calloc((size_t)L + 1, sizeof(int));
    out->lvl_max_n[q] = calloc((size_t)L + 1, sizeof(int));
    if (!out->trsv[q] || !out->lvl_first[q] || !out->lvl_max_n[q]) { chol_set_error("out of memory"); goto done; }
  }
  for (int lvl = 0; lvl < L; lvl++) {
    chol_solve_level sl;
    int r2 = chol_build_solve_level(p, lvl, &sl);
    if (r2) { rc = r2; goto done; }
    for (int q = 0; q < 3; q++) {
      out->lvl_first[q][lvl] = out->n_act[q];
      for (int i = 0; i < sl.n_trsv; i++) {
        const int s = sl.trsv[i].sep;
        if (!(q < 2 ? act[q][s] : (act_fw[s] | act_bw[s]))) continue;
        out->trsv[q][out->n_act[q]++] = sl.trsv[i];
        if (sl.trsv[i].n > out->lvl_max_n[q][lvl]) out->lvl_max_n[q][lvl] = sl.trsv[i].n;
      }
      out->lvl_first[q][lvl + 1] = out->n_act[q];
      if (q < 2) lvl_wide[q][lvl] = out->lvl_max_n[q][lvl];
    }
    chol_solve_level_free(&sl);
  }
  /* the union's positions as ranges, ascending */
  out->range = calloc((size_t)2 * ns + 2, sizeof(int));
  if (!out->range) { chol_set_error("out of memory"); goto done; }
  for (int pos = 0; pos < n;) {
    const int s = p->sep_of_pos[pos], len = p->sep_off[s] + p->sep_size[s] - pos;
    if (len < 1) { chol_set_error("internal: sparse solve: separator %d does not cover position %d", s, pos); rc = CHOLAMD_ERR_INVARIANT; goto done; }
    if (act_fw[s] | act_bw[s]) {
      if (out->n_range > 0 && out->range[2 * out->n_range - 2] + out->range[2 * out->n_range - 1] == pos) out->range[2 * out->n_range - 1] += len;
      else { out->range[2 * out->n_range] = pos; out->range[2 * out->n_range + 1] = len; out->n_range++; }
      out->n_pos += len;
    }
    pos += len;
  }
  /* the pruned steps, items and sources */
  for (int q = 0; q < 2; q++) {
    chol_sdet_step *step = calloc((size_t)w.n_step[q] + 1, sizeof(chol_sdet_step));
    chol_mul_item *item = calloc((size_t)w.n_item[q] + 1, sizeof(chol_mul_item));
    chol_mul_src *src = calloc((size_t)w.n_src[q] + 1, sizeof(chol_mul_src));
    out->w.step[q] = step; out->w.item[q] = item; out->w.src[q] = src;
    if (!step || !item || !src) { chol_set_error("out of memory"); goto done; }
    int nt = 0, ni = 0, nk = 0;
    for (int t = 0; t < w.n_step[q]; t++) {
      const chol_sdet_step *st = &w.step[q][t];
      const int first = ni;
      for (int i = st->item_first; i < st->item_end; i++) {
        const chol_mul_item *it = &w.item[q][i];
        if (!act[q][p->sep_of_pos[it->y_off]]) continue;
        const int k0 = nk;
        for (int e = it->src_first; e < it->src_end; e++) {
          if (q == 0 && !act_fw[p->sep_of_pos[w.src[q][e].z_off]]) continue; /* its factors are exactly zero */
          src[nk++] = w.src[q][e];
        }
        if (nk == k0) continue; /* nothing left to gather: no item */
        const chol_mul_item o = { k0, nk, it->y_off, it->nv };
        item[ni++] = o;
      }
      const int lvl_ok = st->level >= 0 && st->level < L;
      const int keep = st->col0 >= 0 ? lvl_ok && lvl_wide[q][st->level] > st->col0
                                     : ni > first || (st->item_end == st->item_first && lvl_ok && lvl_wide[q][st->level] > 0);
      if (!keep) {
        if (ni > first) { chol_set_error("internal: sparse solve: step %d of direction %d has items but no active separator", t, q); rc = CHOLAMD_ERR_INVARIANT; goto done; }
        continue;
      }
      const chol_sdet_step o = { st->level, st->col0, first, ni };
      step[nt++] = o;
    }
    out->w.n_step[q] = nt; out->w.n_item[q] = ni; out->w.n_src[q] = nk;
  }
  /* the invariants, by walking the sweeps as chol_build_solve_det does, on the active positions alone */
  rc = CHOLAMD_ERR_INVARIANT;
  for (int q = 0; q < 2; q++) {
    memset(solved, 0, (size_t)(n > 0 ? n : 1));
    for (int i = 0; i < n; i++) stamp[i] = -1;
    for (int t = 0; t < out->w.n_step[q]; t++) {
      const chol_sdet_step *st = &out->w.step[q][t];
      for (int i = st->item_first; i < st->item_end; i++) {
        const chol_mul_item *it = &out->w.item[q][i];
        if (it->nv < 1 || it->nv > CHOL_MUL_TILE || it->y_off < 0 || it->y_off + it->nv > n || it->src_end <= it->src_first) { chol_set_error("internal: sparse solve item %d of direction %d is malformed", i, q); goto done; }
        for (int l = 0; l < it->nv; l++) {
          const int pos = it->y_off + l, s = p->sep_of_pos[pos];
          if (!act[q][s] || solved[pos] || stamp[pos] == t || p->level_of[s] != st->level) {
            chol_set_error("internal: sparse solve item %d of direction %d owns position %d, which is inactive, solved, owned twice in the step or outside the step's level", i, q, pos); goto done;
          }
          stamp[pos] = t;
        }
        for (int k = it->src_first; k < it->src_end; k++) {
          const chol_mul_src *s = &out->w.src[q][k];
          if (s->len < 1 || s->a_off < 0 || s->z_off < 0 || s->z_off + s->len > n) { chol_set_error("internal: sparse solve source %d of direction %d leaves the vector", k, q); goto done; }
          const int64_t last = q == 0 ? s->a_off + (it->nv - 1) + (int64_t)(s->len - 1) * s->ld : s->a_off + (s->len - 1) + (int64_t)(it->nv - 1) * s->ld;
          if (last >= p->arena) { chol_set_error("internal: sparse solve source %d of direction %d leaves the arena", k, q); goto done; }
          for (int e = 0; e < s->len; e++)
            if (!act[q][p->sep_of_pos[s->z_off + e]] || !solved[s->z_off + e]) {
              chol_set_error("internal: sparse solve source %d of direction %d reads position %d, which is inactive or not solved yet", k, q, s->z_off + e); goto done;
            }
        }
      }
      if (st->col0 < 0) continue;
      for (int i = out->lvl_first[q][st->level]; i < out->lvl_first[q][st->level + 1]; i++) {
        const chol_trsv_desc *d = &out->trsv[q][i];
        if (d->x_off != p->sep_off[d->sep] || d->n != p->sep_size[d->sep] || !act[q][d->sep]) { chol_set_error("internal: sparse solve: descriptor %d of direction %d is not an active separator's", i, q); goto done; }
        for (int c = st->col0; c < d->n && c < st->col0 + SP; c++) {
          if (solved[d->x_off + c]) { chol_set_error("internal: sparse solve: position %d is solved twice", d->x_off + c); goto done; }
          solved[d->x_off + c] = 1;
        }
      }
      for (int i = st->item_first; i < st->item_end; i++)
        for (int l = 0; l < out->w.item[q][i].nv; l++)
          if (!solved[out->w.item[q][i].y_off + l]) { chol_set_error("internal: sparse solve item %d of direction %d lies outside its step's spans", i, q); goto done; }
    }
    for (int i = 0; i < n; i++)
      if ((solved[i] != 0) != (act[q][p->sep_of_pos[i]] != 0)) { chol_set_error("internal: sparse solve: position %d of direction %d is %s", i, q, solved[i] ? "solved but inactive" : "active but never solved"); goto done; }
  }
  rc = 0;
done:
  free(solved); free(stamp); free(lvl_wide[0]); free(lvl_wide[1]);
  chol_sdet_lists_free(&w);
  if (rc) chol_sparse_lists_free(out);
  return rc;
}

/* masks and lists of a pair of dof lists; pos_in / pos_out: n_in / n_out ints or NULL */
static int sparse_build(const plan_t *p, const char *what, const int *in_dofs, int n_in, const int *out_dofs, int n_out, int *pos_in, int *pos_out, unsigned char **masks,
                        chol_sparse_lists *out)
{
  memset(out, 0, sizeof *out);
  *masks = calloc((size_t)2 * (p->nsep + 1), 1);
  if (!*masks) { chol_set_error("out of memory"); return CHOLAMD_ERR_NOMEM; }
  int rc = chol_sparse_masks(p, what, in_dofs, n_in, out_dofs, n_out, *masks, *masks + p->nsep + 1, pos_in, pos_out);
  if (!rc) rc = chol_build_sparse_det(p, *masks, *masks + p->nsep + 1, out);
  if (rc) { free(*masks); *masks = NULL; }
  return rc;
}
/* one sweep of the pruned lists on the permuted row-major block: the gather of chol_sdet_host_block_gather, the spans of the level's ACTIVE separators only */
static void sparse_host_block_sweep(const plan_t *p, const chol_sparse_lists *w, int which, const double *arena, double *yp)
{
  for (int t = 0; t < w->w.n_step[which]; t++) {
    const chol_sdet_step *st = &w->w.step[which][t];
    chol_sdet_host_block_gather(&w->w, which, st, arena, yp);
    if (st->col0 < 0) continue;
    for (int i = w->lvl_first[which][st->level]; i < w->lvl_first[which][st->level + 1]; i++) chol_sdet_host_block_span(p, w->trsv[which][i].sep, st->col0, which, arena, yp);
  }
}
int cholamd_plan_sparse_solve_host_nrhs(const cholamd_plan *p, const double *arena_host, const int *in_dofs, int n_in, const int *out_dofs, int n_out, int which,
                                        const double *Bs, int64_t ldb, double *Xs, int64_t ldx, int nrhs)
{
  const char *what = "cholamd_plan_sparse_solve_host_nrhs";
  if (!p) { chol_set_error("%s: NULL plan", what); return CHOLAMD_ERR_ARG; }
  if (which != CHOLAMD_HALF_FORWARD && which != CHOLAMD_HALF_BACKWARD && which != -1) { chol_set_error("%s: which = %d is neither CHOLAMD_HALF_FORWARD (0), CHOLAMD_HALF_BACKWARD (1) nor -1 (the whole solve)", what, which); return CHOLAMD_ERR_ARG; }
  if (nrhs < 0) { chol_set_error("%s: nrhs = %d < 0", what, nrhs); return CHOLAMD_ERR_ARG; }
  int *pos = malloc(((size_t)(n_in > 0 ? n_in : 0) + (size_t)(n_out > 0 ? n_out : 0) + 1) * sizeof(int));
  if (!pos) { chol_set_error("out of memory"); return CHOLAMD_ERR_NOMEM; }
  int *pos_in = pos, *pos_out = pos + (n_in > 0 ? n_in : 0);
  unsigned char *masks = NULL;
  chol_sparse_lists w;
  int rc = sparse_build(p, what, in_dofs, n_in, out_dofs, n_out, pos_in, pos_out, &masks, &w);
  if (rc) { free(pos); return rc; }
  double *yp = NULL;
  const int n = p->n;
  rc = CHOLAMD_ERR_ARG;
  if (ldb < n_in || ldx < n_out) { chol_set_error("%s: leading dimensions ldb = %lld, ldx = %lld must be at least n_in = %d, n_out = %d", what, (long long)ldb, (long long)ldx, n_in, n_out); goto done; }
  if (nrhs == 0) { rc = 0; goto done; }
  if (!arena_host || !Bs || !Xs) { chol_set_error("%s: NULL %s", what, !arena_host ? "arena" : !Bs ? "Bs" : "Xs"); goto done; }
  yp = malloc((size_t)(n > 0 ? n : 1) * 32 * sizeof(double));
  if (!yp) { chol_set_error("out of memory"); rc = CHOLAMD_ERR_NOMEM; goto done; }
  for (int64_t i = 0; i < (int64_t)n * 32; i++) yp[i] = (double)NAN; /* what the walk must not read: a read of an inactive row shows in the result */
  for (int c0 = 0; c0 < nrhs; c0 += 32) {
    const int cols = nrhs - c0 < 32 ? nrhs - c0 : 32;
    for (int r = 0; r < w.n_range; r++) memset(yp + (int64_t)w.range[2 * r] * 32, 0, (size_t)w.range[2 * r + 1] * 32 * sizeof(double));
    for (int i = 0; i < n_in; i++)
      for (int j = 0; j < cols; j++) yp[(int64_t)pos_in[i] * 32 + j] = Bs[i + (int64_t)(c0 + j) * ldb]; /* (first: Xs may be Bs) */
    if (which != CHOLAMD_HALF_BACKWARD) sparse_host_block_sweep(p, &w, CHOLAMD_HALF_FORWARD, arena_host, yp);
    if (which != CHOLAMD_HALF_FORWARD) sparse_host_block_sweep(p, &w, CHOLAMD_HALF_BACKWARD, arena_host, yp);
    for (int i = 0; i < n_out; i++)
      for (int j = 0; j < cols; j++) Xs[i + (int64_t)(c0 + j) * ldx] = yp[(int64_t)pos_out[i] * 32 + j];
  }
  rc = 0;
done:
  free(yp); free(pos); free(masks);
  chol_sparse_lists_free(&w);
  return rc;
}
/* out[5 d + 0 .. 4]: active separators, steps, items, sources and entries of L read (items' strips and the active spans' own lower triangles, as
 * cholamd_plan_solve_det_counts counts them) of direction d; out[10]: active positions of the union; out[11]: the ranges they form */
void chol_sparse_counts(const plan_t *p, const chol_sparse_lists *w, int64_t out[12])
{
  (void)p;
  for (int d = 0; d < 2; d++) {
    int64_t entries = 0;
    for (int i = 0; i < w->w.n_item[d]; i++)
      for (int k = w->w.item[d][i].src_first; k < w->w.item[d][i].src_end; k++) entries += (int64_t)w->w.item[d][i].nv * w->w.src[d][k].len;
    for (int i = 0; i < w->n_act[d]; i++)
      for (int c0 = 0; c0 < w->trsv[d][i].n; c0 += CHOL_SDET_SPAN) {
        const int64_t m = w->trsv[d][i].n - c0 < CHOL_SDET_SPAN ? w->trsv[d][i].n - c0 : CHOL_SDET_SPAN;
        entries += m * (m + 1) / 2;
      }
    out[5 * d] = w->n_act[d]; out[5 * d + 1] = w->w.n_step[d]; out[5 * d + 2] = w->w.n_item[d]; out[5 * d + 3] = w->w.n_src[d]; out[5 * d + 4] = entries;
  }
  out[10] = w->n_pos; out[11] = w->n_range;
}
int cholamd_plan_sparse_counts(const cholamd_plan *p, const int *in_dofs, int n_in, const int *out_dofs, int n_out, int64_t out[12])
{
  const char *what = "cholamd_plan_sparse_counts";
  if (!p || !out) { chol_set_error("%s: NULL %s", what, !p ? "plan" : "out"); return CHOLAMD_ERR_ARG; }
  unsigned char *masks = NULL;
  chol_sparse_lists w;
  int rc = sparse_build(p, what, in_dofs, n_in, out_dofs, n_out, NULL, NULL, &masks, &w);
  if (rc) return rc;
  chol_sparse_counts(p, &w, out);
  free(masks);
  chol_sparse_lists_free(&w);
  return 0;
}
int cholamd_plan_sparse_lists(const cholamd_plan *p, const int *in_dofs, int n_in, const int *out_dofs, int n_out, int which, int64_t *steps, int64_t *items, int64_t *srcs)
{
  const char *what = "cholamd_plan_sparse_lists";
  if (!p || !steps || !items || !srcs) { chol_set_error("%s: NULL %s", what, !p ? "plan" : "output"); return CHOLAMD_ERR_ARG; }
  if (which != CHOLAMD_HALF_FORWARD && which != CHOLAMD_HALF_BACKWARD) { chol_set_error("%s: which = %d is neither CHOLAMD_HALF_FORWARD (0) nor CHOLAMD_HALF_BACKWARD (1)", what, which); return CHOLAMD_ERR_ARG; }
  unsigned char *masks = NULL;
  chol_sparse_lists w;
  int rc = sparse_build(p, what, in_dofs, n_in, out_dofs, n_out, NULL, NULL, &masks, &w);
  if (rc) return rc;
  for (int t = 0; t < w.w.n_step[which]; t++) {
    const chol_sdet_step *s = &w.w.step[which][t];
    steps[4 * t] = s->level; steps[4 * t + 1] = s->col0; steps[4 * t + 2] = s->item_first; steps[4 * t + 3] = s->item_end;
  }
  for (int i = 0; i < w.w.n_item[which]; i++) {
    const chol_mul_item *it = &w.w.item[which][i];
    items[4 * i] = it->y_off; items[4 * i + 1] = it->nv; items[4 * i + 2] = it->src_first; items[4 * i + 3] = it->src_end;
  }
  for (int k = 0; k < w.w.n_src[which]; k++) {
    const chol_mul_src *q = &w.w.src[which][k];
    srcs[5 * k] = q->a_off; srcs[5 * k + 1] = q->ld; srcs[5 * k + 2] = q->len; srcs[5 * k + 3] = q->z_off; srcs[5 * k + 4] = q->tri;
  }
  free(masks);
  chol_sparse_lists_free(&w);
  return 0;
}
