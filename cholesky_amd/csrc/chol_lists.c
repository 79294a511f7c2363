/* Device work lists of everything that runs on a finished factor, with their host restatements: the streamed solve, selected inversion, the Schur
 * pieces, the products with the factor, the deterministic solve and its Schur form.  Each builder stands alone; what they share with the factor's
 * schedule (chol_schedule.c) is the partition (chol_split_level, chol_owner_of) and the leaf envelopes (chol_leaf_skylines, chol_leaf_row_first).
 */
#define _GNU_SOURCE
#include <stdlib.h>
#include <string.h>

#include "chol_plan.h"
#include "cholamd.h"

/* ---------------------------------------------------------------------------------------- */
/* solve phase lists (mmat.rg:1394-1479), level by level                                      */
/*   forward  (bottom-up): TRSV per separator, then target-centric GEMV into every ancestor   */
/*   backward (top-down) : per separator gather from all ancestors (GEMV Trans), then TRSV^T  */
/* ---------------------------------------------------------------------------------------- */
/* the stored row runs of a block: maximal runs of consecutive kept 16-row tiles (one run = the whole block without compaction).
 * Calls f(ctx, first row, rows, arena offset of the first row) per run; rows in [lo, hi) only */
typedef struct { int row0, m; int64_t off; } blk_run;
static int block_runs(const chol_block *B, int lo, int hi, blk_run **out)
{
  int cap = 8, n = 0;
  blk_run *r = malloc(cap * sizeof(blk_run));
  if (hi > B->rows) hi = B->rows;
  if (!B->tmap) {
    if (lo < hi) { r[0].row0 = lo; r[0].m = hi - lo; r[0].off = B->off + lo; n = 1; }
  } else
    for (int t = lo / CHOL_NB; t * CHOL_NB < hi; t++) {
      if (B->tmap[t] < 0) continue;
      const int a = t * CHOL_NB > lo ? t * CHOL_NB : lo, b = (t + 1) * CHOL_NB < hi ? (t + 1) * CHOL_NB : hi;
      if (n > 0 && r[n - 1].row0 + r[n - 1].m == a) { r[n - 1].m += b - a; continue; }
      if (n == cap) { cap *= 2; r = realloc(r, cap * sizeof(blk_run)); }
      r[n].row0 = a; r[n].m = b - a; r[n].off = chol_block_row(B, a); n++;
    }
  *out = r;
  return n;
}

int cholamd_plan_solve_counts(const cholamd_plan *p, int level, int rank, int world, int64_t out[5])
{ /* host-side view of one rank's solve lists of a level: separators, (ancestor, separator) row runs, forward / backward row chunks, columns solved */
  if (level < 0 || level >= p->levels || world < 1 || (world & (world - 1)) || rank < 0 || rank >= world || chol_split_level(world) > p->levels - 1) { chol_set_error("bad solve partition"); return CHOLAMD_ERR_ARG; }
  chol_solve_level w;
  int rc = chol_build_solve_level_part(p, level, rank, world, &w);
  if (rc) return rc;
  out[0] = w.n_trsv; out[1] = w.n_bw; out[2] = w.n_ifw; out[3] = w.n_ibw; out[4] = 0;
  for (int i = 0; i < w.n_trsv; i++) out[4] += w.trsv[i].n;
  chol_solve_level_free(&w);
  return 0;
}
int chol_build_solve_level(const plan_t *p, int level, chol_solve_level *w) { return chol_build_solve_level_part(p, level, 0, 1, w); }
int cholamd_plan_solve_skips(const cholamd_plan *p, int level, int *seps, int *runs)
{
  if (!p || level < 0 || level >= p->levels || !seps || !runs) { chol_set_error("solve_skips: bad arguments"); return CHOLAMD_ERR_ARG; }
  chol_solve_level w;
  int rc = chol_build_solve_level(p, level, &w);
  if (rc) return rc;
  for (int t = 0; t < w.n_trsv; t++) { seps[3 * t] = w.trsv[t].x_off; seps[3 * t + 1] = w.trsv[t].n; seps[3 * t + 2] = w.trsv[t].band; }
  for (int q = 0; q < w.n_bw; q++) { runs[5 * q] = w.bw[q].x_off; runs[5 * q + 1] = w.bw[q].m; runs[5 * q + 2] = w.bw[q].y_off; runs[5 * q + 3] = w.bw[q].n; runs[5 * q + 4] = w.bw[q].c_lo; }
  chol_solve_level_free(&w);
  return 0;
}
/* the same for rank `rank` of `world` (distributed solve, mmat.rg:1394-1479 sharded like the factorisation): below the cut only the separators of
 * the rank's own subtrees -- their TRSVs and their panels into every ancestor, the shared top included; the levels above the cut complete (every
 * rank holds the whole factored top and solves it redundantly: only vectors travel) */
int chol_build_solve_level_part(const plan_t *p, int level, int rank, int world, chol_solve_level *w)
{
  memset(w, 0, sizeof *w);
  const int cut = chol_split_level(world);
#define SOLVE_MINE(s_) (world <= 1 || level < cut || chol_owner_of(p, (s_), world) == rank)
  const int h0 = 1 << level, h1 = (1 << (level + 1)) - 1, cnt = h1 - h0 + 1;
  int capb = cnt * (level > 0 ? level : 1);
  w->trsv = malloc(cnt * sizeof(chol_trsv_desc));
  w->bw_start = malloc((cnt + 1) * sizeof(int));
  w->bw = malloc((size_t)capb * sizeof(chol_gemv_desc));
  for (int h = h0; h <= h1; h++) {
    int s = p->tree[h];
    if (!SOLVE_MINE(s)) continue;
    chol_trsv_desc t = { p->panel_off[s], p->sep_size[s], p->panel_ld[s], p->sep_off[s], s, p->dinv_off[s], 0 };
    if (p->sep_size[s] > w->max_n) w->max_n = p->sep_size[s];
    w->bw_start[w->n_trsv] = w->n_bw;
    w->trsv[w->n_trsv++] = t;
    for (int hp = h / 2; hp >= 1; hp /= 2) {
      int par = p->tree[hp];
      const chol_block *B = &p->blk[BIDX(p, par, s)];
      if (B->rows == 0 || B->cols == 0) continue;
      blk_run *rr; const int nr = block_runs(B, 0, B->rows, &rr); /* one descriptor per stored row run */
      for (int q = 0; q < nr; q++)
        for (int r0 = 0; r0 < rr[q].m; r0 += CHOL_SOLVE_BW_ROWS) { /* rows of a run are consecutive in memory and in the ancestor's vector */
          if (w->n_bw == capb) { capb *= 2; w->bw = realloc(w->bw, (size_t)capb * sizeof(chol_gemv_desc)); }
          const int m = rr[q].m - r0 < CHOL_SOLVE_BW_ROWS ? rr[q].m - r0 : CHOL_SOLVE_BW_ROWS;
          chol_gemv_desc g = { rr[q].off + r0, m, B->cols, B->ld, p->sep_off[par] + rr[q].row0 + r0, p->sep_off[s], 0 };
          w->bw[w->n_bw++] = g;
        }
      free(rr);
    }
  }
  w->bw_start[w->n_trsv] = w->n_bw;
  w->max_rows_under_span = w->max_n;
  int **rfirst = NULL; /* leaf level: first entry of every panel row */
  if (level == p->levels - 1 && w->n_trsv > 0 && !getenv("CHOLAMD_SOLVE_NO_BAND")) { /* leaves: the element band of the tile skyline (a tile (ti, tj) with tj < sky[ti] is zero) */
    rfirst = chol_leaf_row_first(p);
    for (int t = 0; t < w->n_trsv; t++) { /* ... and the first non-zero column of every row run into the ancestors */
      const int s = w->trsv[t].sep;
      if (!rfirst[s]) continue;
      for (int q = w->bw_start[t]; q < w->bw_start[t + 1]; q++) {
        const int pr = (int)((w->bw[q].a_off - p->panel_off[s]) % p->panel_ld[s]);
        int f = w->bw[q].n;
        for (int r = 0; r < w->bw[q].m; r++) if (rfirst[s][pr + r] < f) f = rfirst[s][pr + r];
        w->bw[q].c_lo = f & ~15;
      }
    }
    unsigned char **sky = chol_leaf_skylines(p);
    w->max_rows_under_span = 0;
    for (int t = 0; t < w->n_trsv; t++) {
      const int s = w->trsv[t].sep, n = w->trsv[t].n;
      int band = 0;
      if (sky[s]) {
        int md = 0;
        for (int i = 0; i * CHOL_NB < n; i++) if (i - sky[s][i] > md) md = i - sky[s][i];
        band = CHOL_NB * md + CHOL_NB - 1;
        if (band >= n) band = 0;
      }
      w->trsv[t].band = band;
      if ((band > 0 ? band : n) > w->max_rows_under_span) w->max_rows_under_span = band > 0 ? band : n;
    }
    w->banded = w->max_rows_under_span <= 256; /* (SSPAN of chol_solve.hip) */
    chol_free_skylines(sky, p->nsep);
  }
  /* forward: for every ancestor separator `par` (levels above), chunks of 256 rows; a source = the stored rows of a block inside the
   * chunk (y_off = first row of the run, relative to the target separator) */
  int cap = 16, capg = 16;
  w->fw = malloc(cap * sizeof(chol_gemv_desc));
  w->grp_start = malloc((capg + 1) * sizeof(int));
  w->grp_rows = malloc(2 * capg * sizeof(int));
  for (int pl = level - 1; pl >= 0; pl--)
    for (int hp = 1 << pl; hp < (1 << (pl + 1)); hp++) {
      int par = p->tree[hp];
      if (p->sep_size[par] == 0) continue;
      for (int row0 = 0; row0 < p->sep_size[par]; row0 += 256) {
        if (w->n_grp == capg) { capg *= 2; w->grp_start = realloc(w->grp_start, (capg + 1) * sizeof(int)); w->grp_rows = realloc(w->grp_rows, 2 * capg * sizeof(int)); }
        w->grp_start[w->n_grp] = w->n_fw;
        w->grp_rows[2 * w->n_grp] = row0; w->grp_rows[2 * w->n_grp + 1] = p->sep_off[par];
        w->n_grp++;
        for (int h = hp << (level - pl); h < ((hp + 1) << (level - pl)); h++) {
          int s = p->tree[h];
          if (!SOLVE_MINE(s)) continue;
          const chol_block *B = &p->blk[BIDX(p, par, s)];
          if (B->rows == 0 || B->cols == 0) continue;
          blk_run *rr; const int nr = block_runs(B, row0, row0 + 256, &rr);
          for (int q = 0; q < nr; q++) {
            if (w->n_fw == cap) { cap *= 2; w->fw = realloc(w->fw, cap * sizeof(chol_gemv_desc)); }
            chol_gemv_desc g = { rr[q].off, rr[q].m, B->cols, B->ld, p->sep_off[s], rr[q].row0, 0 };
            w->fw[w->n_fw++] = g;
          }
          free(rr);
        }
      }
    }
  w->grp_start[w->n_grp] = w->n_fw;
  /* row chunks of the blocks for the source-centric kernels of the driver-level solve */
  { /* backward: per separator, 64-column chunks x ranges of its row runs holding about R rows; R as large as keeps CHOL_SOLVE_BW_ITEMS workgroups */
    int64_t R = (int64_t)1 << 30;
    int n = 0, *it = NULL;
    for (;;) {
      n = 0;
      for (int pass = 0; pass < 2; pass++) { /* count, then fill */
        int k = 0;
        for (int t = 0; t < w->n_trsv; t++) {
          const int nc = (w->trsv[t].n + CHOL_SOLVE_BW_COLS - 1) / CHOL_SOLVE_BW_COLS;
          for (int q0 = w->bw_start[t]; q0 < w->bw_start[t + 1];) {
            int q1 = q0; int64_t rows = 0;
            while (q1 < w->bw_start[t + 1] && (q1 == q0 || rows + w->bw[q1].m <= R)) rows += w->bw[q1++].m;
            if (pass) for (int c = 0; c < nc; c++) { it[4 * k] = q0; it[4 * k + 1] = q1; it[4 * k + 2] = c * CHOL_SOLVE_BW_COLS; it[4 * k + 3] = 0; k++; }
            else k += nc;
            q0 = q1;
          }
        }
        if (!pass) {
          n = k;
          if (n < CHOL_SOLVE_BW_ITEMS && R > CHOL_SOLVE_BW_ROWS) break; /* too few: halve R and count again */
          it = malloc((size_t)(n > 0 ? 4 * n : 4) * sizeof(int));
        }
      }
      if (it) break;
      R = R > ((int64_t)1 << 20) ? ((int64_t)1 << 20) : R / 2;
    }
    w->ibw = it; w->n_ibw = n;
  }
  for (int pass = 0; pass < 1; pass++) {
    const int rows = pass ? CHOL_SOLVE_BW_ROWS : CHOL_SOLVE_FW_ROWS;
    int n = 0;
    for (int i = 0; i < w->n_bw; i++) n += ((w->bw[i].m + rows - 1) / rows) * ((w->bw[i].n + CHOL_SOLVE_COLS - 1) / CHOL_SOLVE_COLS);
    int *it = malloc((size_t)(n > 0 ? 4 * n : 4) * sizeof(int)), k = 0;
    for (int t = 0; t < w->n_trsv; t++) {
      const int s = w->trsv[t].sep;
      for (int i = w->bw_start[t]; i < w->bw_start[t + 1]; i++)
        for (int c0 = 0; c0 < w->bw[i].n; c0 += CHOL_SOLVE_COLS)
          for (int r0 = 0; r0 < w->bw[i].m; r0 += rows) {
            int f = 0;
            if (rfirst && rfirst[s]) { /* the first non-zero column of these rows */
              const int pr = (int)((w->bw[i].a_off - p->panel_off[s]) % p->panel_ld[s]);
              f = w->bw[i].n;
              for (int r = r0; r < r0 + rows && r < w->bw[i].m; r++) if (rfirst[s][pr + r] < f) f = rfirst[s][pr + r];
              f &= ~15;
            }
            it[4 * k] = i; it[4 * k + 1] = r0; it[4 * k + 2] = c0; it[4 * k + 3] = f; k++;
          }
    }
    if (pass) { w->ibw = it; w->n_ibw = n; } else { w->ifw = it; w->n_ifw = n; }
  }
  if (rfirst) { for (int s = 1; s <= p->nsep; s++) free(rfirst[s]); free(rfirst); }
#undef SOLVE_MINE
  return 0;
}

void chol_solve_level_free(chol_solve_level *w)
{
  free(w->trsv); free(w->fw); free(w->grp_start); free(w->grp_rows); free(w->bw); free(w->bw_start); free(w->ifw); free(w->ibw);
  memset(w, 0, sizeof *w);
}

/* The diagonal of the factor (cholamd_factor_diag / _logdet): the TRSV descriptors of every level in ONE list, ordered by their position in the permuted
 * vector, with prefix[i] = columns before descriptor i (prefix[count] = n).  Element j of descriptor i is arena[a_off + j (lda + 1)] and belongs to
 * permuted position x_off + j.  Sorts `list` in place; fails unless the descriptors tile [0, n) exactly once. */
static int diag_by_pos(const void *a, const void *b)
{
  const chol_trsv_desc *x = a, *y = b;
  return x->x_off < y->x_off ? -1 : x->x_off > y->x_off;
}
int chol_diag_list(const plan_t *p, chol_trsv_desc *list, int count, int *prefix)
{
  qsort(list, (size_t)count, sizeof *list, diag_by_pos);
  int at = 0;
  for (int i = 0; i < count; i++) {
    if (list[i].x_off != at || list[i].n < 0 || list[i].lda < list[i].n || list[i].a_off < 0 || list[i].a_off + (int64_t)list[i].n * list[i].lda > p->arena) {
      chol_set_error("internal: the diagonal descriptors do not tile the permuted vector (descriptor %d of separator %d at %d, expected %d)", i, list[i].sep, list[i].x_off, at);
      return CHOLAMD_ERR_INVARIANT;
    }
    prefix[i] = at;
    at += list[i].n;
  }
  prefix[count] = at;
  if (at != p->n) { chol_set_error("internal: the diagonal descriptors cover %d of %d positions", at, p->n); return CHOLAMD_ERR_INVARIANT; }
  return 0;
}
int cholamd_plan_diag_list(const cholamd_plan *p, int64_t *a_off, int *cols, int *lda, int *x_off, int *sep, int *prefix)
{
  if (!p) { chol_set_error("cholamd_plan_diag_list: NULL plan"); return CHOLAMD_ERR_ARG; }
  chol_trsv_desc *list = malloc((size_t)p->nsep * sizeof *list);
  int *pre = malloc(((size_t)p->nsep + 1) * sizeof(int)), count = 0, rc = 0;
  for (int lvl = 0; lvl < p->levels && !rc; lvl++) {
    chol_solve_level w;
    rc = chol_build_solve_level(p, lvl, &w);
    if (rc) break;
    if (count + w.n_trsv > p->nsep) { chol_set_error("internal: more diagonal descriptors than separators"); rc = CHOLAMD_ERR_INVARIANT; }
    else { memcpy(list + count, w.trsv, (size_t)w.n_trsv * sizeof *list); count += w.n_trsv; }
    chol_solve_level_free(&w);
  }
  if (!rc) rc = chol_diag_list(p, list, count, pre);
  for (int i = 0; i < count && !rc; i++) {
    if (a_off) a_off[i] = list[i].a_off;
    if (cols) cols[i] = list[i].n;
    if (lda) lda[i] = list[i].lda;
    if (x_off) x_off[i] = list[i].x_off;
    if (sep) sep[i] = list[i].sep;
  }
  if (!rc && prefix) memcpy(prefix, pre, ((size_t)count + 1) * sizeof(int));
  free(list); free(pre);
  return rc ? rc : count;
}

/* ---------------------------------------------------------------------------------------- */
/* selected inversion: the gather lists of one tree level (chol_plan.h at chol_selinv_level)  */
/* ---------------------------------------------------------------------------------------- */
static int selinv_by_blocks(const void *a, const void *b)
{
  const chol_selinv_sep *x = a, *y = b;
  return x->nblk != y->nblk ? (x->nblk > y->nblk ? -1 : 1) : (x->sep < y->sep ? -1 : x->sep > y->sep);
}
void chol_selinv_level_free(chol_selinv_level *w)
{
  free(w->sep); free(w->tile); free(w->chain_ld); free(w->chain_pos0); free(w->rowoff);
  memset(w, 0, sizeof *w);
}
int chol_build_selinv_level(const plan_t *p, int level, chol_selinv_level *out)
{
  memset(out, 0, sizeof *out);
  out->level = level;
  if (level < 0 || level >= p->levels) { chol_set_error("selected inversion: level %d of %d", level, p->levels); return CHOLAMD_ERR_ARG; }
  const int h_lo = 1 << level, h_hi = (2 << level) - 1 < p->nsep ? (2 << level) - 1 : p->nsep;
  const int nchain = level + 1;
  int ns = 0;
  int64_t ntile = 0;
  for (int h = h_lo; h <= h_hi; h++) {
    const int s = p->tree[h];
    if (p->sep_size[s] <= 0) continue;
    ns++;
    for (int a = h; a >= 1; a /= 2) ntile += (p->sep_size[p->tree[a]] + CHOL_NB - 1) / CHOL_NB;
  }
  out->sep = calloc((size_t)(ns > 0 ? ns : 1), sizeof *out->sep);
  out->tile = calloc((size_t)(ntile > 0 ? ntile : 1), sizeof *out->tile);
  out->chain_ld = calloc((size_t)(ns > 0 ? ns : 1) * nchain, sizeof(int));
  out->chain_pos0 = calloc((size_t)(ns > 0 ? ns : 1) * nchain, sizeof(int));
  out->rowoff = malloc((size_t)(ntile > 0 ? ntile : 1) * nchain * sizeof(int64_t));
  if (!out->sep || !out->tile || !out->chain_ld || !out->chain_pos0 || !out->rowoff) { chol_selinv_level_free(out); chol_set_error("out of memory"); return CHOLAMD_ERR_NOMEM; }
  for (int h = h_lo; h <= h_hi; h++) {
    const int s = p->tree[h];
    if (p->sep_size[s] <= 0) continue;
    chol_selinv_sep *d = &out->sep[out->n_sep++];
    d->sep = s; d->panel_off = p->panel_off[s]; d->ld = p->panel_ld[s]; d->w = p->sep_size[s]; d->prows = p->panel_rows[s];
    d->nblk = (d->w + CHOL_SELINV_W - 1) / CHOL_SELINV_W;
    d->nown = (d->w + CHOL_NB - 1) / CHOL_NB;
    d->tile_first = out->n_tile; d->chain_first = out->n_chain; d->nchain = nchain; d->rowoff_first = out->n_rowoff;
    int k = 0;
    for (int a = h; a >= 1; a /= 2, k++) { /* the chain, bottom up: the panels Z is gathered from */
      out->chain_ld[out->n_chain + k] = p->panel_ld[p->tree[a]];
      out->chain_pos0[out->n_chain + k] = p->sep_off[p->tree[a]];
    }
    out->n_chain += nchain;
    k = 0;
    for (int a = h; a >= 1; a /= 2, k++) { /* the tiles of panel(s) in storage order */
      const int anc = p->tree[a];
      const chol_block *B = chol_plan_block(p, anc, s);
      if (!B) { chol_selinv_level_free(out); chol_set_error("internal: no block (%d, %d)", anc, s); return CHOLAMD_ERR_INVARIANT; }
      for (int r0 = 0; r0 < B->rows; r0 += CHOL_NB) {
        const int64_t ro = chol_block_row(B, r0);
        if (ro < 0) continue;
        chol_selinv_tile *t = &out->tile[out->n_tile];
        t->q0 = (int)(ro - p->panel_off[s]); t->nrows = B->rows - r0 < CHOL_NB ? B->rows - r0 : CHOL_NB; t->pos0 = p->sep_off[anc] + r0; t->k = k;
        int64_t *ro_t = &out->rowoff[out->n_rowoff];
        int k2 = 0;
        for (int a2 = h; a2 >= 1; a2 /= 2, k2++) { /* where the tile's rows lie in the panels of the chain: the extend-add's relation, read instead of written */
          const chol_block *B2 = k2 <= k ? chol_plan_block(p, anc, p->tree[a2]) : NULL;
          ro_t[k2] = B2 ? chol_block_row(B2, r0) : -1;
        }
        out->n_tile++; out->n_rowoff += nchain;
      }
    }
    d->ntile = out->n_tile - d->tile_first;
    d->ws_off = out->ws_doubles;
    out->ws_doubles += 2 * (int64_t)d->prows * CHOL_SELINV_W + CHOL_SELINV_W * CHOL_SELINV_W;
    if (d->nblk > out->max_nblk) out->max_nblk = d->nblk;
    if (d->ntile > out->max_tiles) out->max_tiles = d->ntile;
  }
  qsort(out->sep, (size_t)out->n_sep, sizeof *out->sep, selinv_by_blocks);
  return 0;
}

/* the arena offset of Z(i, j) by the rule of the kernels; i, j: (tile, row inside the tile) of one separator's list */
static int64_t selinv_offset(const chol_selinv_level *w, const chol_selinv_sep *d, int ta, int ra, int tb, int rb)
{
  if (ta < tb || (ta == tb && ra < rb)) { int t = ta; ta = tb; tb = t; t = ra; ra = rb; rb = t; }
  const chol_selinv_tile *B = &w->tile[d->tile_first + tb];
  const int64_t base = w->rowoff[d->rowoff_first + (int64_t)ta * d->nchain + B->k];
  if (base < 0) return -1;
  return base + ra + (int64_t)(B->pos0 + rb - w->chain_pos0[d->chain_first + B->k]) * w->chain_ld[d->chain_first + B->k];
}
int cholamd_plan_selinv_blocks(const cholamd_plan *p, int sep)
{
  if (!p || sep < 1 || sep > p->nsep) { chol_set_error("cholamd_plan_selinv_blocks: no separator %d", sep); return CHOLAMD_ERR_ARG; }
  return (p->sep_size[sep] + CHOL_SELINV_W - 1) / CHOL_SELINV_W;
}
int cholamd_plan_selinv_front(const cholamd_plan *p, int sep, int block, int cap, int cols[2], int *pos, int64_t *off)
{
  if (!p || sep < 1 || sep > p->nsep) { chol_set_error("cholamd_plan_selinv_front: no separator %d", sep); return CHOLAMD_ERR_ARG; }
  const int nblk = (p->sep_size[sep] + CHOL_SELINV_W - 1) / CHOL_SELINV_W;
  if (block < 0 || block >= nblk) { chol_set_error("cholamd_plan_selinv_front: separator %d has %d column blocks, not block %d", sep, nblk, block); return CHOLAMD_ERR_ARG; }
  chol_selinv_level w;
  int rc = chol_build_selinv_level(p, p->level_of[sep], &w);
  if (rc) return rc;
  const chol_selinv_sep *d = NULL;
  for (int i = 0; i < w.n_sep; i++) if (w.sep[i].sep == sep) d = &w.sep[i];
  if (!d) { chol_selinv_level_free(&w); chol_set_error("internal: separator %d is not in the lists of its level", sep); return CHOLAMD_ERR_INVARIANT; }
  const int j0 = block * CHOL_SELINV_W, j1 = j0 + CHOL_SELINV_W < d->w ? j0 + CHOL_SELINV_W : d->w;
  const int t0 = j1 == d->w ? d->nown : j1 / CHOL_NB;
  int m = 0;
  for (int t = t0; t < d->ntile; t++) m += w.tile[d->tile_first + t].nrows;
  if (cols) { cols[0] = p->sep_off[sep] + j0; cols[1] = j1 - j0; }
  if (pos || off) {
    if (m > cap || m > CHOLAMD_SELINV_FRONT_MAX) {
      chol_selinv_level_free(&w);
      chol_set_error("cholamd_plan_selinv_front: %d rows below block %d of separator %d (room for %d, at most %d)", m, block, sep, cap, CHOLAMD_SELINV_FRONT_MAX);
      return CHOLAMD_ERR_ARG;
    }
    int *tl = malloc((size_t)(m > 0 ? m : 1) * 2 * sizeof(int));
    if (!tl) { chol_selinv_level_free(&w); chol_set_error("out of memory"); return CHOLAMD_ERR_NOMEM; }
    int i = 0;
    for (int t = t0; t < d->ntile; t++)
      for (int r = 0; r < w.tile[d->tile_first + t].nrows; r++, i++) {
        tl[2 * i] = t; tl[2 * i + 1] = r;
        if (pos) pos[i] = w.tile[d->tile_first + t].pos0 + r;
      }
    if (off)
      for (int a = 0; a < m; a++)
        for (int b = 0; b < m; b++) off[(size_t)a * m + b] = selinv_offset(&w, d, tl[2 * a], tl[2 * a + 1], tl[2 * b], tl[2 * b + 1]);
    free(tl);
  }
  chol_selinv_level_free(&w);
  return m;
}

/* ---------------------------------------------------------------------------------------- */
/* Schur complement on the top k levels of the tree (include/cholamd.h at cholamd_schur)       */
/* ---------------------------------------------------------------------------------------- */
int chol_schur_range(const cholamd_plan *p, int k, int *t0_out)
{
  if (!p) { chol_set_error("schur: NULL plan"); return CHOLAMD_ERR_ARG; }
  if (k < 1 || k > p->levels - 1 || (1 << k) - 1 > p->nsep) {
    chol_set_error("schur: k = %d kept levels, the tree of %d levels allows 1 .. %d", k, p->levels, p->levels - 1);
    return CHOLAMD_ERR_ARG;
  }
  const int nk = (1 << k) - 1;
  int m = 0, lo = p->n;
  for (int h = 1; h <= nk; h++) {
    const int s = p->tree[h];
    if (p->sep_size[s] <= 0) continue;
    m += p->sep_size[s];
    if (p->sep_off[s] < lo) lo = p->sep_off[s];
  }
  if (lo != p->n - m) { /* the kept separators are the last labels: a contiguous tail of the permuted order */
    chol_set_error("schur: the top %d levels hold %d dofs but start at permuted position %d of %d", k, m, lo, p->n);
    return CHOLAMD_ERR_INVARIANT;
  }
  if (t0_out) *t0_out = lo;
  return m;
}
int64_t chol_schur_pieces(const cholamd_plan *p, int k, int with_empty, int chunk, int64_t cap, chol_schur_desc *out)
{
  int t0 = 0;
  const int m = chol_schur_range(p, k, &t0);
  if (m < 0) return m;
  const int nk = (1 << k) - 1;
  int64_t cnt = 0;
  for (int hc = 1; hc <= nk; hc++) {
    const int c = p->tree[hc], wc = p->sep_size[c];
    if (wc <= 0) continue;
    for (int hr = 1; hr <= nk; hr++) {
      const int r = p->tree[hr], wr = p->sep_size[r];
      if (wr <= 0 || p->sep_off[r] < p->sep_off[c]) continue; /* the lower block triangle */
      const chol_block *B = chol_plan_block(p, r, c);
      if (!B && !with_empty) continue; /* not ancestor and descendant: structurally zero */
      if (B && (B->rows != wr || B->cols != wc || B->lo_x != p->sep_off[r] || B->lo_y != p->sep_off[c])) {
        chol_set_error("internal: block (%d, %d) does not span its separators", r, c);
        return CHOLAMD_ERR_INVARIANT;
      }
      const int diag = r == c;
      for (int i0 = 0; i0 < wr; i0 += CHOL_NB) {
        const int rows = wr - i0 < CHOL_NB ? wr - i0 : CHOL_NB;
        const int64_t row = B ? chol_block_row(B, i0) : -1;
        if (row < 0 && !with_empty) continue; /* a tile the row compaction dropped */
        const int ncols = diag ? i0 + rows : wc; /* a diagonal block stores its lower triangle */
        if (row >= 0 && (row + rows - 1 + (int64_t)(ncols - 1) * B->ld >= p->arena)) {
          chol_set_error("internal: tile %d of block (%d, %d) leaves the arena", i0 / CHOL_NB, r, c);
          return CHOLAMD_ERR_INVARIANT;
        }
        const int step = chunk > 0 ? chunk : ncols;
        for (int j0 = 0; j0 < ncols; j0 += step, cnt++) {
          if (cnt >= cap) continue;
          chol_schur_desc *q = &out[cnt];
          q->off = row < 0 ? -1 : row + (int64_t)j0 * B->ld;
          q->ld = B ? B->ld : 0;
          q->rows = rows; q->cols = ncols - j0 < step ? ncols - j0 : step;
          q->row0 = p->sep_off[r] - t0 + i0; q->col0 = p->sep_off[c] - t0 + j0;
          q->diag = diag;
        }
      }
    }
  }
  return cnt;
}
int cholamd_plan_schur_size(const cholamd_plan *p, int k) { return chol_schur_range(p, k, NULL); }
int cholamd_plan_schur_dofs(const cholamd_plan *p, int k, int *dofs_out)
{
  int t0 = 0;
  const int m = chol_schur_range(p, k, &t0);
  if (m < 0) return m;
  if (!dofs_out) { chol_set_error("cholamd_plan_schur_dofs: NULL dofs_out"); return CHOLAMD_ERR_ARG; }
  memcpy(dofs_out, p->perm + t0, (size_t)m * sizeof(int));
  return m;
}
int cholamd_plan_schur_list(const cholamd_plan *p, int k, int64_t cap, int64_t *out)
{
  const int64_t cnt = chol_schur_pieces(p, k, 0, 0, 0, NULL);
  if (cnt < 0) return (int)cnt;
  if (cnt > INT32_MAX) { chol_set_error("cholamd_plan_schur_list: %lld records", (long long)cnt); return CHOLAMD_ERR_ARG; }
  if (cap <= 0 || !out) return (int)cnt;
  chol_schur_desc *q = malloc((size_t)(cnt > 0 ? cnt : 1) * sizeof *q);
  if (!q) { chol_set_error("out of memory"); return CHOLAMD_ERR_NOMEM; }
  chol_schur_pieces(p, k, 0, 0, cnt, q);
  for (int64_t i = 0; i < cnt && i < cap; i++) {
    int64_t *o = out + CHOLAMD_SCHUR_RECORD * i;
    o[0] = q[i].off; o[1] = q[i].ld; o[2] = q[i].rows; o[3] = q[i].cols; o[4] = q[i].row0; o[5] = q[i].col0; o[6] = q[i].diag;
  }
  free(q);
  return (int)cnt;
}
int cholamd_plan_schur_host(const cholamd_plan *p, int k, const double *arena_host, double *S, int64_t lds)
{
  const int m = chol_schur_range(p, k, NULL);
  if (m < 0) return m;
  if (!arena_host || !S) { chol_set_error("cholamd_plan_schur_host: NULL %s", !arena_host ? "arena" : "S"); return CHOLAMD_ERR_ARG; }
  if (lds < m) { chol_set_error("cholamd_plan_schur_host: lds = %lld < m = %d", (long long)lds, m); return CHOLAMD_ERR_ARG; }
  const int64_t cnt = chol_schur_pieces(p, k, 0, 0, 0, NULL);
  if (cnt < 0) return (int)cnt;
  chol_schur_desc *q = malloc((size_t)(cnt > 0 ? cnt : 1) * sizeof *q);
  if (!q) { chol_set_error("out of memory"); return CHOLAMD_ERR_NOMEM; }
  chol_schur_pieces(p, k, 0, 0, cnt, q);
  for (int j = 0; j < m; j++) memset(S + (int64_t)j * lds, 0, (size_t)m * sizeof(double));
  for (int64_t e = 0; e < cnt; e++)
    for (int j = 0; j < q[e].cols; j++)
      for (int i = 0; i < q[e].rows; i++) {
        const int R = q[e].row0 + i, C = q[e].col0 + j;
        if (q[e].diag && R < C) continue;
        const double v = arena_host[q[e].off + i + (int64_t)j * q[e].ld];
        S[R + (int64_t)C * lds] = v;
        S[C + (int64_t)R * lds] = v;
      }
  free(q);
  return 0;
}

/* ---------------------------------------------------------------------------------------- */
/* forward product with the factor (cholamd_multiply_half): the owner lists of the whole tree  */
/* (chol_plan.h at chol_mul_lists) and their host restatement                                  */
/* ---------------------------------------------------------------------------------------- */
#define MUL_TRI_OFF (1 << 30)
typedef struct { chol_mul_item *item; chol_mul_src *src; int n_item, cap_item, n_src, cap_src, fail; } mul_build;
static void mul_push_src(mul_build *b, int64_t a_off, int ld, int len, int z_off, int tri)
{
  if (len <= 0 || b->fail) return;
  if (b->n_src == b->cap_src) {
    if (b->cap_src > (1 << 29)) { b->fail = 1; return; }
    b->cap_src = b->cap_src ? 2 * b->cap_src : 256;
    chol_mul_src *q = realloc(b->src, (size_t)b->cap_src * sizeof *q);
    if (!q) { b->fail = 1; return; }
    b->src = q;
  }
  const chol_mul_src s = { a_off, ld, len, z_off, tri };
  b->src[b->n_src++] = s;
}
static void mul_open_item(mul_build *b, int y_off, int nv)
{
  if (b->fail) return;
  if (b->n_item == b->cap_item) {
    b->cap_item = b->cap_item ? 2 * b->cap_item : 256;
    chol_mul_item *q = realloc(b->item, (size_t)b->cap_item * sizeof *q);
    if (!q) { b->fail = 1; return; }
    b->item = q;
  }
  const chol_mul_item it = { b->n_src, b->n_src, y_off, nv };
  b->item[b->n_item++] = it;
}
static void mul_close_item(mul_build *b) { if (!b->fail) b->item[b->n_item - 1].src_end = b->n_src; }

void chol_mul_lists_free(chol_mul_lists *w)
{
  for (int q = 0; q < 2; q++) { free(w->item[q]); free(w->src[q]); }
  memset(w, 0, sizeof *w);
}
int chol_build_multiply(const plan_t *p, chol_mul_lists *out)
{
  memset(out, 0, sizeof *out);
  const int ns = p->nsep, T = CHOL_MUL_TILE;
  int *band = calloc((size_t)ns + 1, sizeof(int));
  int **rfirst = NULL;
  if (!band) { chol_set_error("out of memory"); return CHOLAMD_ERR_NOMEM; }
  if (!getenv("CHOLAMD_SOLVE_NO_BAND")) { /* the structural zeros of the leaves, as the solve lists know them (chol_build_solve_level_part) */
    rfirst = chol_leaf_row_first(p);
    unsigned char **sky = chol_leaf_skylines(p);
    for (int s = 1; s <= ns; s++) {
      if (!sky[s]) continue;
      const int n = p->sep_size[s];
      int md = 0;
      for (int i = 0; i * CHOL_NB < n; i++) if (i - sky[s][i] > md) md = i - sky[s][i];
      band[s] = CHOL_NB * md + CHOL_NB - 1;
      if (band[s] >= n) band[s] = 0;
    }
    chol_free_skylines(sky, ns);
  }
  mul_build fw = { 0 }, bw = { 0 };
  int *desc = NULL, cap_desc = 0; /* blocks (s, descendant) that exist, of the separator at hand */
  for (int h = 1; h <= ns; h++) {
    const int s = p->tree[h], n = p->sep_size[s], ld = p->panel_ld[s], x0 = p->sep_off[s];
    if (n <= 0) continue;
    /* FORWARD: the 16-row chunks of s gather from the diagonal block and from every descendant's panel.  The descendants whose panel stores rows of s
     * are found once per separator (level by level downwards: the order of the sums), the chunks then walk that list */
    int nd = 0;
    for (int64_t lo = 2 * (int64_t)h, hi = 2 * (int64_t)h + 1; lo <= ns; lo *= 2, hi = 2 * hi + 1)
      for (int64_t hd = lo; hd <= hi && hd <= ns; hd++) {
        const int bi = BIDX(p, s, p->tree[hd]);
        if (bi < 0 || p->blk[bi].rows == 0 || p->blk[bi].cols == 0) continue;
        if (nd == cap_desc) {
          cap_desc = cap_desc ? 2 * cap_desc : 64;
          int *q = realloc(desc, (size_t)cap_desc * sizeof(int));
          if (!q) { fw.fail = 1; break; }
          desc = q;
        }
        desc[nd++] = bi;
      }
    for (int r0 = 0; r0 < n; r0 += T) {
      const int nv = n - r0 < T ? n - r0 : T;
      mul_open_item(&fw, x0 + r0, nv);
      const int c0 = band[s] > 0 && r0 > band[s] ? (r0 - band[s]) & ~(T - 1) : 0;
      mul_push_src(&fw, p->panel_off[s] + r0 + (int64_t)c0 * ld, ld, r0 + nv - c0, x0 + c0, r0 - c0);
      for (int e = 0; e < nd; e++) {
        const chol_block *B = &p->blk[desc[e]];
        const int sd = B->c;
        if (r0 >= B->rows) continue;
        const int64_t off = chol_block_row(B, r0);
        if (off < 0) continue;
        int c_lo = 0;
        if (rfirst && rfirst[sd]) {
          const int pr = (int)((off - p->panel_off[sd]) % p->panel_ld[sd]);
          c_lo = B->cols;
          for (int i = 0; i < nv; i++) if (rfirst[sd][pr + i] < c_lo) c_lo = rfirst[sd][pr + i];
          c_lo &= ~(T - 1);
        }
        mul_push_src(&fw, off + (int64_t)c_lo * B->ld, B->ld, B->cols - c_lo, p->sep_off[sd] + c_lo, MUL_TRI_OFF);
      }
      mul_close_item(&fw);
    }
    /* BACKWARD: the 16-column chunks of s read their own columns of panel(s): the triangle, then the stored row runs into the ancestors */
    for (int c0 = 0; c0 < n; c0 += T) {
      const int nv = n - c0 < T ? n - c0 : T;
      mul_open_item(&bw, x0 + c0, nv);
      const int r1 = band[s] > 0 && c0 + nv + band[s] < n ? c0 + nv + band[s] : n;
      mul_push_src(&bw, p->panel_off[s] + c0 + (int64_t)c0 * ld, ld, r1 - c0, x0 + c0, 0);
      for (int hp = h / 2; hp >= 1; hp /= 2) {
        const int par = p->tree[hp];
        const int bi = BIDX(p, par, s);
        if (bi < 0) continue;
        const chol_block *B = &p->blk[bi];
        if (B->rows == 0 || B->cols == 0) continue;
        blk_run *rr; const int nr = block_runs(B, 0, B->rows, &rr);
        for (int q = 0; q < nr; q++) {
          if (rfirst && rfirst[s]) {
            const int pr = (int)((rr[q].off - p->panel_off[s]) % ld);
            int f = n;
            for (int r = 0; r < rr[q].m; r++) if (rfirst[s][pr + r] < f) f = rfirst[s][pr + r];
            if (c0 + nv <= (f & ~(T - 1))) continue; /* the run is zero in these columns */
          }
          mul_push_src(&bw, rr[q].off + (int64_t)c0 * B->ld, B->ld, rr[q].m, p->sep_off[par] + rr[q].row0, -T);
        }
        free(rr);
      }
      mul_close_item(&bw);
    }
  }
  if (rfirst) { for (int s = 1; s <= ns; s++) free(rfirst[s]); free(rfirst); }
  free(band); free(desc);
  out->item[0] = fw.item; out->n_item[0] = fw.n_item; out->src[0] = fw.src; out->n_src[0] = fw.n_src;
  out->item[1] = bw.item; out->n_item[1] = bw.n_item; out->src[1] = bw.src; out->n_src[1] = bw.n_src;
  if (fw.fail || bw.fail) { chol_mul_lists_free(out); chol_set_error("multiply lists: out of memory or more than 2^30 sources"); return CHOLAMD_ERR_NOMEM; }
  /* every permuted position has exactly one owner in each direction, every source lies inside the arena */
  for (int w = 0; w < 2; w++) {
    int64_t owned = 0;
    for (int i = 0; i < out->n_item[w]; i++) owned += out->item[w][i].nv;
    if (owned != p->n) { chol_set_error("internal: the multiply items own %lld of %d positions", (long long)owned, p->n); chol_mul_lists_free(out); return CHOLAMD_ERR_INVARIANT; }
    for (int i = 0; i < out->n_item[w]; i++)
      for (int k = out->item[w][i].src_first; k < out->item[w][i].src_end; k++) {
        const chol_mul_src *q = &out->src[w][k];
        const int nv = out->item[w][i].nv;
        const int64_t last = w == 0 ? q->a_off + (nv - 1) + (int64_t)(q->len - 1) * q->ld : q->a_off + (q->len - 1) + (int64_t)(nv - 1) * q->ld;
        if (q->a_off < 0 || q->z_off < 0 || q->z_off + q->len > p->n || last >= p->arena) {
          chol_set_error("internal: multiply source %d of direction %d leaves the arena or the vector", k, w); chol_mul_lists_free(out); return CHOLAMD_ERR_INVARIANT;
        }
      }
  }
  return 0;
}
int cholamd_plan_multiply_host(const cholamd_plan *p, const double *arena_host, int which, const double *z, double *y)
{
  if (!p || !arena_host || !z || !y) { chol_set_error("cholamd_plan_multiply_host: NULL %s", !p ? "plan" : !arena_host ? "arena" : !z ? "z" : "y"); return CHOLAMD_ERR_ARG; }
  if (which != CHOLAMD_HALF_FORWARD && which != CHOLAMD_HALF_BACKWARD) { chol_set_error("cholamd_plan_multiply_host: which = %d is neither CHOLAMD_HALF_FORWARD (0) nor CHOLAMD_HALF_BACKWARD (1)", which); return CHOLAMD_ERR_ARG; }
  chol_mul_lists w;
  int rc = chol_build_multiply(p, &w);
  if (rc) return rc;
  const int n = p->n;
  double *zp = malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
  if (!zp) { chol_mul_lists_free(&w); chol_set_error("out of memory"); return CHOLAMD_ERR_NOMEM; }
  for (int i = 0; i < n; i++) zp[i] = z[p->perm[i]];
  for (int i = 0; i < w.n_item[which]; i++) {
    const chol_mul_item *it = &w.item[which][i];
    double acc[CHOL_MUL_TILE] = { 0 };
    for (int k = it->src_first; k < it->src_end; k++) {
      const chol_mul_src *q = &w.src[which][k];
      for (int e = 0; e < q->len; e++) {
        const double ze = zp[q->z_off + e];
        for (int l = 0; l < it->nv; l++) {
          if (which == CHOLAMD_HALF_FORWARD ? e - l > q->tri : e < q->tri + l) continue; /* outside the lower triangle: not part of the factor */
          acc[l] += arena_host[which == CHOLAMD_HALF_FORWARD ? q->a_off + l + (int64_t)e * q->ld : q->a_off + e + (int64_t)l * q->ld] * ze;
        }
      }
    }
    for (int l = 0; l < it->nv; l++) y[p->perm[it->y_off + l]] = acc[l];
  }
  free(zp);
  chol_mul_lists_free(&w);
  return 0;
}
/* One direction of the block product on the host: out (n x 32, permuted, row-major) = L zp or L^T zp with the block kernel's own partition of a source --
 * chunks of CHOL_MULN_KSTEP steps dealt to CHOL_MULN_WAVES partial tiles by chol_muln_wave, every operand of a chunk read (clamped) and selected by
 * chol_muln_elem as k_multiply_nrhs does, the partial tiles added in wave order */
static void mul_host_block(const chol_mul_lists *w, int which, const double *arena, const double *zp, double *out)
{
  enum { T = CHOL_MUL_TILE, W = 32 };
  double acc[CHOL_MULN_WAVES][T][W]; /* the waves' partial tiles (16 KB) */
  for (int i = 0; i < w->n_item[which]; i++) {
    const chol_mul_item *it = &w->item[which][i];
    memset(acc, 0, sizeof acc);
    for (int s = it->src_first; s < it->src_end; s++) {
      const chol_mul_src *q = &w->src[which][s];
      for (int c = 0; c * CHOL_MULN_KSTEP < q->len; c++) {
        double (*a)[W] = acc[chol_muln_wave(s - it->src_first, c)];
        for (int k = c * CHOL_MULN_KSTEP; k < (c + 1) * CHOL_MULN_KSTEP; k++)
          for (int l = 0; l < T; l++) {
            int meant;
            const double v = arena[chol_muln_elem(q, which, it->nv, l, k, &meant)]; /* read whether meant or not: the clamp keeps it inside the strip */
            if (!meant) continue;
            const double *zr = zp + (int64_t)(q->z_off + k) * W;
            for (int j = 0; j < W; j++) a[l][j] += v * zr[j];
          }
      }
    }
    for (int l = 0; l < it->nv; l++)
      for (int j = 0; j < W; j++) {
        double sum = acc[0][l][j];
        for (int wv = 1; wv < CHOL_MULN_WAVES; wv++) sum += acc[wv][l][j];
        out[(int64_t)(it->y_off + l) * W + j] = sum;
      }
  }
}
int cholamd_plan_multiply_host_nrhs(const cholamd_plan *p, const double *arena_host, int which, const double *Z, int64_t ldz, double *Y, int64_t ldy, int nrhs)
{
  const char *what = "cholamd_plan_multiply_host_nrhs";
  if (!p) { chol_set_error("%s: NULL plan", what); return CHOLAMD_ERR_ARG; }
  if (which != CHOLAMD_HALF_FORWARD && which != CHOLAMD_HALF_BACKWARD && which != -1) { chol_set_error("%s: which = %d is neither CHOLAMD_HALF_FORWARD (0), CHOLAMD_HALF_BACKWARD (1) nor -1 (the full product)", what, which); return CHOLAMD_ERR_ARG; }
  const int n = p->n;
  if (nrhs < 0) { chol_set_error("%s: nrhs = %d < 0", what, nrhs); return CHOLAMD_ERR_ARG; }
  if (ldz < n || ldy < n) { chol_set_error("%s: leading dimensions ldz = %lld, ldy = %lld must be at least n = %d", what, (long long)ldz, (long long)ldy, n); return CHOLAMD_ERR_ARG; }
  if (nrhs == 0) return 0;
  if (!arena_host || !Z || !Y) { chol_set_error("%s: NULL %s", what, !arena_host ? "arena" : !Z ? "Z" : "Y"); return CHOLAMD_ERR_ARG; }
  chol_mul_lists w;
  int rc = chol_build_multiply(p, &w);
  if (rc) return rc;
  const size_t blk = (size_t)(n > 0 ? n : 1) * 32;
  double *zp = malloc(blk * sizeof(double)), *wp = malloc(blk * sizeof(double));
  if (!zp || !wp) { free(zp); free(wp); chol_mul_lists_free(&w); chol_set_error("out of memory"); return CHOLAMD_ERR_NOMEM; }
  for (int c0 = 0; c0 < nrhs; c0 += 32) {
    const int cols = nrhs - c0 < 32 ? nrhs - c0 : 32;
    for (int i = 0; i < n; i++)
      for (int j = 0; j < 32; j++) zp[(int64_t)i * 32 + j] = j < cols ? Z[p->perm[i] + (int64_t)(c0 + j) * ldz] : 0.0; /* (first: Y may be Z) */
    const double *res = wp;
    if (which == -1) {
      mul_host_block(&w, CHOLAMD_HALF_BACKWARD, arena_host, zp, wp);
      mul_host_block(&w, CHOLAMD_HALF_FORWARD, arena_host, wp, zp);
      res = zp;
    } else mul_host_block(&w, which, arena_host, zp, wp);
    for (int i = 0; i < n; i++)
      for (int j = 0; j < cols; j++) Y[p->perm[i] + (int64_t)(c0 + j) * ldy] = res[(int64_t)i * 32 + j];
  }
  free(zp); free(wp);
  chol_mul_lists_free(&w);
  return 0;
}
int cholamd_plan_multiply_counts(const cholamd_plan *p, int64_t out[6])
{
  if (!p || !out) { chol_set_error("cholamd_plan_multiply_counts: NULL %s", !p ? "plan" : "out"); return CHOLAMD_ERR_ARG; }
  chol_mul_lists w;
  int rc = chol_build_multiply(p, &w);
  if (rc) return rc;
  for (int d = 0; d < 2; d++) {
    int64_t entries = 0;
    for (int i = 0; i < w.n_item[d]; i++)
      for (int k = w.item[d][i].src_first; k < w.item[d][i].src_end; k++) {
        const chol_mul_src *q = &w.src[d][k];
        for (int l = 0; l < w.item[d][i].nv; l++) { /* steps of line l that are meant (chol_plan.h at chol_mul_src) */
          const int64_t lo = d == 0 ? 0 : (q->tri + l > 0 ? q->tri + l : 0), hi = d == 0 ? ((int64_t)q->tri + l + 1 < q->len ? (int64_t)q->tri + l + 1 : q->len) : q->len;
          if (hi > lo) entries += hi - lo;
        }
      }
    out[3 * d] = w.n_item[d]; out[3 * d + 1] = w.n_src[d]; out[3 * d + 2] = entries;
  }
  chol_mul_lists_free(&w);
  return 0;
}

/* ---------------------------------------------------------------------------------------- */
/* deterministic streamed solve (option solve_deterministic): the step lists of both sweeps   */
/* (chol_plan.h at chol_sdet_lists) and their host restatement                                */
/* ---------------------------------------------------------------------------------------- */
void chol_sdet_lists_free(chol_sdet_lists *w)
{
  for (int q = 0; q < 2; q++) { free(w->step[q]); free(w->item[q]); free(w->src[q]); }
  memset(w, 0, sizeof *w);
}
/* The lists are derived from the multiply lists, so leaf bands, leaf envelopes (c_lo) and row compaction are honoured exactly as chol_build_multiply honours
 * them: the first source of a multiply item is its diagonal-block source, the others are what the solve gathers from outside the block; the part of the
 * diagonal-block source outside the item's own span becomes the in-block source. */
int chol_build_solve_det(const plan_t *p, chol_sdet_lists *out)
{
  memset(out, 0, sizeof *out);
  const int ns = p->nsep, L = p->levels, T = CHOL_MUL_TILE, SP = CHOL_SDET_SPAN;
  chol_mul_lists m;
  int rc = chol_build_multiply(p, &m);
  if (rc) return rc;
  int *nspan = calloc((size_t)L + 1, sizeof(int)), *first_item = calloc((size_t)L + 2, sizeof(int)); /* per level: spans of the widest separator, first multiply item */
  int *stamp = malloc((size_t)(p->n > 0 ? p->n : 1) * sizeof(int));
  unsigned char *solved = calloc((size_t)(p->n > 0 ? p->n : 1), 1);
  mul_build b[2] = { { 0 }, { 0 } };
  int total = 0;
  rc = CHOLAMD_ERR_NOMEM;
  if (!nspan || !first_item || !stamp || !solved) { chol_set_error("out of memory"); goto done; }
  { /* the items of both multiply lists come separator by separator in heap order, one per 16 positions */
    int it = 0;
    for (int h = 1; h <= ns; h++) {
      int lvl = 0;
      while ((h >> (lvl + 1)) > 0) lvl++;
      const int n = p->sep_size[p->tree[h]];
      if (lvl >= L) { chol_set_error("internal: heap index %d lies below the %d levels of the tree", h, L); rc = CHOLAMD_ERR_INVARIANT; goto done; }
      if ((n + SP - 1) / SP > nspan[lvl]) nspan[lvl] = (n + SP - 1) / SP;
      if (h == (1 << lvl)) first_item[lvl] = it;
      for (int r0 = 0; r0 < n; r0 += T, it++)
        if (it >= m.n_item[0] || it >= m.n_item[1] || m.item[0][it].y_off != p->sep_off[p->tree[h]] + r0 || m.item[1][it].y_off != m.item[0][it].y_off) {
          chol_set_error("internal: multiply item %d is not chunk %d of separator %d", it, r0 / T, p->tree[h]); rc = CHOLAMD_ERR_INVARIANT; goto done;
        }
    }
    if (it != m.n_item[0] || it != m.n_item[1]) { chol_set_error("internal: %d chunks, %d / %d multiply items", it, m.n_item[0], m.n_item[1]); rc = CHOLAMD_ERR_INVARIANT; goto done; }
  }
  for (int lvl = 0; lvl < L; lvl++) if (nspan[lvl] > 0) total += 1 + nspan[lvl];
  for (int q = 0; q < 2; q++) {
    out->step[q] = calloc((size_t)(total > 0 ? total : 1), sizeof(chol_sdet_step));
    if (!out->step[q]) { chol_set_error("out of memory"); goto done; }
    int t = 0;
    for (int li = 0; li < L; li++) { /* FORWARD: leaves first, span 0 first; BACKWARD: root first, the last span first; the level's outside gather in front */
      const int lvl = q == 0 ? L - 1 - li : li;
      if (nspan[lvl] == 0) continue;
      const chol_sdet_step lead = { lvl, -1, 0, 0 };
      out->step[q][t++] = lead;
      for (int ki = 0; ki < nspan[lvl]; ki++) {
        const chol_sdet_step st = { lvl, (q == 0 ? ki : nspan[lvl] - 1 - ki) * SP, 0, 0 };
        out->step[q][t++] = st;
      }
    }
    out->n_step[q] = t;
  }
  for (int q = 0; q < 2; q++)
    for (int t = 0; t < total; t++) {
      chol_sdet_step *st = &out->step[q][t];
      st->item_first = b[q].n_item;
      int it = first_item[st->level];
      for (int h = 1 << st->level; h < (1 << (st->level + 1)) && h <= ns; h++) {
        const int s = p->tree[h], n = p->sep_size[s], x0 = p->sep_off[s], nch = (n + T - 1) / T;
        const int c_lo = st->col0 < 0 ? 0 : st->col0 / T, c_hi = st->col0 < 0 ? nch : (st->col0 + SP) / T;
        for (int c = c_lo; c < nch && c < c_hi; c++) {
          const chol_mul_item *mi = &m.item[q][it + c];
          if (st->col0 < 0) { /* everything but the diagonal-block source (the first one of a multiply item) */
            if (mi->src_end - mi->src_first <= 1) continue; /* nothing to gather: no item */
            mul_open_item(&b[q], mi->y_off, mi->nv);
            for (int e = mi->src_first + 1; e < mi->src_end; e++) mul_push_src(&b[q], m.src[q][e].a_off, m.src[q][e].ld, m.src[q][e].len, m.src[q][e].z_off, m.src[q][e].tri);
            mul_close_item(&b[q]);
            continue;
          }
          const chol_mul_src *q0 = &m.src[q][mi->src_first]; /* the diagonal-block source */
          const int r0 = c * T;
          int in_len, in_z; int64_t in_off;
          if (q == 0) { /* columns [first column of the band, col0) of the chunk's rows */
            in_len = st->col0 - (q0->z_off - x0); in_z = q0->z_off; in_off = q0->a_off;
          } else {      /* rows [col0 + span, end of the band) of the chunk's columns */
            in_len = r0 + q0->len - (st->col0 + SP); in_z = x0 + st->col0 + SP; in_off = q0->a_off + (st->col0 + SP - r0);
          }
          if (in_len <= 0) continue;
          mul_open_item(&b[q], mi->y_off, mi->nv);
          mul_push_src(&b[q], in_off, q0->ld, in_len, in_z, q == 0 ? MUL_TRI_OFF : -T);
          mul_close_item(&b[q]);
        }
        it += nch;
      }
      st->item_end = b[q].n_item;
    }
  for (int q = 0; q < 2; q++) {
    out->item[q] = b[q].item; out->n_item[q] = b[q].n_item; out->src[q] = b[q].src; out->n_src[q] = b[q].n_src;
    b[q].item = NULL; b[q].src = NULL;
  }
  if (b[0].fail || b[1].fail) { chol_set_error("solve lists: out of memory or more than 2^30 sources"); goto done; }
  /* the invariants, by walking the sweeps: a source is inside the arena and solved before its step, an item owns positions of its step's level (of its
   * step's spans) that are not solved yet and that nobody else of the step owns, the spans solve every position exactly once */
  rc = CHOLAMD_ERR_INVARIANT;
  for (int q = 0; q < 2; q++) {
    memset(solved, 0, (size_t)(p->n > 0 ? p->n : 1));
    for (int i = 0; i < p->n; i++) stamp[i] = -1;
    for (int t = 0; t < total; t++) {
      const chol_sdet_step *st = &out->step[q][t];
      for (int i = st->item_first; i < st->item_end; i++) {
        const chol_mul_item *it = &out->item[q][i];
        if (it->nv < 1 || it->nv > T || it->y_off < 0 || it->y_off + it->nv > p->n || it->src_end <= it->src_first) { chol_set_error("internal: solve item %d of direction %d is malformed", i, q); goto done; }
        for (int l = 0; l < it->nv; l++) {
          const int pos = it->y_off + l, hs = p->heap_of[p->sep_of_pos[pos]];
          if (solved[pos] || stamp[pos] == t || hs < (1 << st->level) || hs >= (1 << (st->level + 1))) {
            chol_set_error("internal: solve item %d of direction %d owns position %d, which is solved, owned twice in the step or outside the step's level", i, q, pos); goto done;
          }
          stamp[pos] = t;
        }
        for (int k = it->src_first; k < it->src_end; k++) {
          const chol_mul_src *s = &out->src[q][k];
          const int64_t last = q == 0 ? s->a_off + (it->nv - 1) + (int64_t)(s->len - 1) * s->ld : s->a_off + (s->len - 1) + (int64_t)(it->nv - 1) * s->ld;
          if (s->len < 1 || s->a_off < 0 || s->z_off < 0 || s->z_off + s->len > p->n || last >= p->arena) { chol_set_error("internal: solve source %d of direction %d leaves the arena or the vector", k, q); goto done; }
          for (int e = 0; e < s->len; e++)
            if (!solved[s->z_off + e]) { chol_set_error("internal: solve source %d of direction %d reads position %d before it is solved", k, q, s->z_off + e); goto done; }
        }
      }
      if (st->col0 < 0) continue;
      for (int h = 1 << st->level; h < (1 << (st->level + 1)) && h <= ns; h++) {
        const int s = p->tree[h], n = p->sep_size[s];
        for (int i = st->col0; i < n && i < st->col0 + SP; i++) {
          if (solved[p->sep_off[s] + i]) { chol_set_error("internal: position %d is solved twice", p->sep_off[s] + i); goto done; }
          solved[p->sep_off[s] + i] = 1;
        }
      }
      for (int i = st->item_first; i < st->item_end; i++)
        for (int l = 0; l < out->item[q][i].nv; l++)
          if (!solved[out->item[q][i].y_off + l]) { chol_set_error("internal: solve item %d of direction %d lies outside its step's spans", i, q); goto done; }
    }
    for (int i = 0; i < p->n; i++) if (!solved[i]) { chol_set_error("internal: position %d is never solved", i); goto done; }
  }
  rc = 0;
done:
  free(nspan); free(first_item); free(stamp); free(solved);
  for (int q = 0; q < 2; q++) { free(b[q].item); free(b[q].src); }
  chol_mul_lists_free(&m);
  if (rc) chol_sdet_lists_free(out);
  return rc;
}
/* one sweep over a host arena in permuted coordinates: per step the gathers, item by item and source by source in list order, then the span of every
 * separator of the level by substitution inside the span's own triangle (rows / columns of the span only; the lower triangle only) */
static void sdet_host_sweep(const plan_t *p, const chol_sdet_lists *w, int which, const double *arena, double *y)
{
  for (int t = 0; t < w->n_step[which]; t++) {
    const chol_sdet_step *st = &w->step[which][t];
    for (int i = st->item_first; i < st->item_end; i++) {
      const chol_mul_item *it = &w->item[which][i];
      double acc[CHOL_MUL_TILE] = { 0 };
      for (int k = it->src_first; k < it->src_end; k++) {
        const chol_mul_src *q = &w->src[which][k];
        for (int e = 0; e < q->len; e++) {
          const double ze = y[q->z_off + e];
          for (int l = 0; l < it->nv; l++)
            acc[l] += arena[which == CHOLAMD_HALF_FORWARD ? q->a_off + l + (int64_t)e * q->ld : q->a_off + e + (int64_t)l * q->ld] * ze;
        }
      }
      for (int l = 0; l < it->nv; l++) y[it->y_off + l] -= acc[l];
    }
    if (st->col0 < 0) continue; /* the level's outside gather: no span */
    for (int h = 1 << st->level; h < (1 << (st->level + 1)) && h <= p->nsep; h++) {
      const int s = p->tree[h], n = p->sep_size[s], ld = p->panel_ld[s];
      if (n <= st->col0) continue;
      const int n1 = n < st->col0 + CHOL_SDET_SPAN ? n : st->col0 + CHOL_SDET_SPAN;
      const double *Lm = arena + p->panel_off[s];
      double *x = y + p->sep_off[s];
      if (which == CHOLAMD_HALF_FORWARD)
        for (int i = st->col0; i < n1; i++) {
          double v = x[i];
          for (int j = st->col0; j < i; j++) v -= Lm[i + (int64_t)j * ld] * x[j];
          x[i] = v / Lm[i + (int64_t)i * ld];
        }
      else
        for (int i = n1 - 1; i >= st->col0; i--) {
          double v = x[i];
          for (int j = i + 1; j < n1; j++) v -= Lm[j + (int64_t)i * ld] * x[j];
          x[i] = v / Lm[i + (int64_t)i * ld];
        }
    }
  }
}
int cholamd_plan_solve_det_host(const cholamd_plan *p, const double *arena_host, int which, const double *b, double *x)
{
  if (!p || !arena_host || !b || !x) { chol_set_error("cholamd_plan_solve_det_host: NULL %s", !p ? "plan" : !arena_host ? "arena" : !b ? "b" : "x"); return CHOLAMD_ERR_ARG; }
  if (which != CHOLAMD_HALF_FORWARD && which != CHOLAMD_HALF_BACKWARD && which != -1) { chol_set_error("cholamd_plan_solve_det_host: which = %d is neither CHOLAMD_HALF_FORWARD (0), CHOLAMD_HALF_BACKWARD (1) nor -1 (the whole solve)", which); return CHOLAMD_ERR_ARG; }
  chol_sdet_lists w;
  int rc = chol_build_solve_det(p, &w);
  if (rc) return rc;
  const int n = p->n;
  double *y = malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
  if (!y) { chol_sdet_lists_free(&w); chol_set_error("out of memory"); return CHOLAMD_ERR_NOMEM; }
  for (int i = 0; i < n; i++) y[i] = b[p->perm[i]]; /* (first: x may be b) */
  if (which != CHOLAMD_HALF_BACKWARD) sdet_host_sweep(p, &w, CHOLAMD_HALF_FORWARD, arena_host, y);
  if (which != CHOLAMD_HALF_FORWARD) sdet_host_sweep(p, &w, CHOLAMD_HALF_BACKWARD, arena_host, y);
  for (int i = 0; i < n; i++) x[p->perm[i]] = y[i];
  free(y);
  chol_sdet_lists_free(&w);
  return 0;
}
/* The block form (option solve_deterministic_block of the device; chol_solve_det.hip at k_solve_det_gather_nrhs): one sweep over a host arena on the
 * permuted ROW-major block yp (n x 32).  A gather has the kernel's own partition -- chol_muln_wave deals a source's chunks of CHOL_MULN_KSTEP steps to four
 * partial tiles, chol_muln_elem gives the operand (read clamped, skipped where it is not meant), the four partial sums of an element are added in wave
 * order and subtracted from the owner's value.  A span is solved by substitution inside its own lower triangle, column by column of the block, as
 * sdet_host_sweep does (the device's span kernel sums in another order: the host walk does not return the device's bits).  Every column of the block
 * goes through its own scalar operations: no column's result depends on another's. */
void chol_sdet_host_block_gather(const chol_sdet_lists *w, int which, const chol_sdet_step *st, const double *arena, double *yp)
{
  enum { T = CHOL_MUL_TILE, W = 32 };
  double acc[CHOL_MULN_WAVES][T][W];
  for (int i = st->item_first; i < st->item_end; i++) {
    const chol_mul_item *it = &w->item[which][i];
    memset(acc, 0, sizeof acc);
    for (int s = it->src_first; s < it->src_end; s++) {
      const chol_mul_src *q = &w->src[which][s];
      for (int c = 0; c * CHOL_MULN_KSTEP < q->len; c++) {
        double (*a)[W] = acc[chol_muln_wave(s - it->src_first, c)];
        for (int k = c * CHOL_MULN_KSTEP; k < (c + 1) * CHOL_MULN_KSTEP; k++)
          for (int l = 0; l < T; l++) {
            int meant;
            const double v = arena[chol_muln_elem(q, which, it->nv, l, k, &meant)]; /* read whether meant or not: the clamp keeps it inside the strip */
            if (!meant) continue;
            const double *zr = yp + (int64_t)(q->z_off + k) * W;
            for (int j = 0; j < W; j++) a[l][j] += v * zr[j];
          }
      }
    }
    for (int l = 0; l < it->nv; l++)
      for (int j = 0; j < W; j++) {
        double sum = acc[0][l][j];
        for (int wv = 1; wv < CHOL_MULN_WAVES; wv++) sum += acc[wv][l][j];
        yp[(int64_t)(it->y_off + l) * W + j] -= sum;
      }
  }
}
void chol_sdet_host_block_span(const plan_t *p, int s, int col0, int which, const double *arena, double *yp)
{
  enum { W = 32 };
  const int n = p->sep_size[s], ld = p->panel_ld[s];
  if (n <= col0) return;
  const int n1 = n < col0 + CHOL_SDET_SPAN ? n : col0 + CHOL_SDET_SPAN;
  const double *Lm = arena + p->panel_off[s];
  double *x = yp + (int64_t)p->sep_off[s] * W;
  for (int c = 0; c < W; c++)
    if (which == CHOLAMD_HALF_FORWARD)
      for (int i = col0; i < n1; i++) {
        double v = x[(int64_t)i * W + c];
        for (int j = col0; j < i; j++) v -= Lm[i + (int64_t)j * ld] * x[(int64_t)j * W + c];
        x[(int64_t)i * W + c] = v / Lm[i + (int64_t)i * ld];
      }
    else
      for (int i = n1 - 1; i >= col0; i--) {
        double v = x[(int64_t)i * W + c];
        for (int j = i + 1; j < n1; j++) v -= Lm[j + (int64_t)i * ld] * x[(int64_t)j * W + c];
        x[(int64_t)i * W + c] = v / Lm[i + (int64_t)i * ld];
      }
}
static void sdet_host_block_sweep(const plan_t *p, const chol_sdet_lists *w, int which, const double *arena, double *yp)
{
  for (int t = 0; t < w->n_step[which]; t++) {
    const chol_sdet_step *st = &w->step[which][t];
    chol_sdet_host_block_gather(w, which, st, arena, yp);
    if (st->col0 < 0) continue; /* the level's outside gather: no span */
    for (int h = 1 << st->level; h < (1 << (st->level + 1)) && h <= p->nsep; h++) chol_sdet_host_block_span(p, p->tree[h], st->col0, which, arena, yp);
  }
}
int cholamd_plan_solve_det_host_nrhs(const cholamd_plan *p, const double *arena_host, int which, const double *B, int64_t ldb, double *X, int64_t ldx, int nrhs)
{
  const char *what = "cholamd_plan_solve_det_host_nrhs";
  if (!p) { chol_set_error("%s: NULL plan", what); return CHOLAMD_ERR_ARG; }
  if (which != CHOLAMD_HALF_FORWARD && which != CHOLAMD_HALF_BACKWARD && which != -1) { chol_set_error("%s: which = %d is neither CHOLAMD_HALF_FORWARD (0), CHOLAMD_HALF_BACKWARD (1) nor -1 (the whole solve)", what, which); return CHOLAMD_ERR_ARG; }
  const int n = p->n;
  if (nrhs < 0) { chol_set_error("%s: nrhs = %d < 0", what, nrhs); return CHOLAMD_ERR_ARG; }
  if (ldb < n || ldx < n) { chol_set_error("%s: leading dimensions ldb = %lld, ldx = %lld must be at least n = %d", what, (long long)ldb, (long long)ldx, n); return CHOLAMD_ERR_ARG; }
  if (nrhs == 0) return 0;
  if (!arena_host || !B || !X) { chol_set_error("%s: NULL %s", what, !arena_host ? "arena" : !B ? "B" : "X"); return CHOLAMD_ERR_ARG; }
  chol_sdet_lists w;
  int rc = chol_build_solve_det(p, &w);
  if (rc) return rc;
  double *yp = malloc((size_t)(n > 0 ? n : 1) * 32 * sizeof(double));
  if (!yp) { chol_sdet_lists_free(&w); chol_set_error("out of memory"); return CHOLAMD_ERR_NOMEM; }
  for (int c0 = 0; c0 < nrhs; c0 += 32) {
    const int cols = nrhs - c0 < 32 ? nrhs - c0 : 32;
    for (int i = 0; i < n; i++)
      for (int j = 0; j < 32; j++) yp[(int64_t)i * 32 + j] = j < cols ? B[p->perm[i] + (int64_t)(c0 + j) * ldb] : 0.0; /* (first: X may be B) */
    if (which != CHOLAMD_HALF_BACKWARD) sdet_host_block_sweep(p, &w, CHOLAMD_HALF_FORWARD, arena_host, yp);
    if (which != CHOLAMD_HALF_FORWARD) sdet_host_block_sweep(p, &w, CHOLAMD_HALF_BACKWARD, arena_host, yp);
    for (int i = 0; i < n; i++)
      for (int j = 0; j < cols; j++) X[p->perm[i] + (int64_t)(c0 + j) * ldx] = yp[(int64_t)i * 32 + j];
  }
  free(yp);
  chol_sdet_lists_free(&w);
  return 0;
}
int cholamd_plan_solve_det_counts(const cholamd_plan *p, int64_t out[8])
{
  if (!p || !out) { chol_set_error("cholamd_plan_solve_det_counts: NULL %s", !p ? "plan" : "out"); return CHOLAMD_ERR_ARG; }
  chol_sdet_lists w;
  int rc = chol_build_solve_det(p, &w);
  if (rc) return rc;
  for (int d = 0; d < 2; d++) {
    int64_t entries = 0;
    for (int i = 0; i < w.n_item[d]; i++)
      for (int k = w.item[d][i].src_first; k < w.item[d][i].src_end; k++) entries += (int64_t)w.item[d][i].nv * w.src[d][k].len;
    for (int s = 1; s <= p->nsep; s++) /* the spans' own lower triangles */
      for (int c0 = 0; c0 < p->sep_size[s]; c0 += CHOL_SDET_SPAN) {
        const int64_t m = p->sep_size[s] - c0 < CHOL_SDET_SPAN ? p->sep_size[s] - c0 : CHOL_SDET_SPAN;
        entries += m * (m + 1) / 2;
      }
    out[4 * d] = w.n_step[d]; out[4 * d + 1] = w.n_item[d]; out[4 * d + 2] = w.n_src[d]; out[4 * d + 3] = entries;
  }
  chol_sdet_lists_free(&w);
  return 0;
}
int cholamd_plan_solve_det_lists(const cholamd_plan *p, int which, int64_t *steps, int64_t *items, int64_t *srcs)
{
  if (!p || !steps || !items || !srcs) { chol_set_error("cholamd_plan_solve_det_lists: NULL %s", !p ? "plan" : "output"); return CHOLAMD_ERR_ARG; }
  if (which != CHOLAMD_HALF_FORWARD && which != CHOLAMD_HALF_BACKWARD) { chol_set_error("cholamd_plan_solve_det_lists: which = %d is neither CHOLAMD_HALF_FORWARD (0) nor CHOLAMD_HALF_BACKWARD (1)", which); return CHOLAMD_ERR_ARG; }
  chol_sdet_lists w;
  int rc = chol_build_solve_det(p, &w);
  if (rc) return rc;
  for (int t = 0; t < w.n_step[which]; t++) {
    const chol_sdet_step *s = &w.step[which][t];
    steps[4 * t] = s->level; steps[4 * t + 1] = s->col0; steps[4 * t + 2] = s->item_first; steps[4 * t + 3] = s->item_end;
  }
  for (int i = 0; i < w.n_item[which]; i++) {
    const chol_mul_item *it = &w.item[which][i];
    items[4 * i] = it->y_off; items[4 * i + 1] = it->nv; items[4 * i + 2] = it->src_first; items[4 * i + 3] = it->src_end;
  }
  for (int k = 0; k < w.n_src[which]; k++) {
    const chol_mul_src *q = &w.src[which][k];
    srcs[5 * k] = q->a_off; srcs[5 * k + 1] = q->ld; srcs[5 * k + 2] = q->len; srcs[5 * k + 3] = q->z_off; srcs[5 * k + 4] = q->tri;
  }
  chol_sdet_lists_free(&w);
  return 0;
}

/* ---------------------------------------------------------------------------------------- */
/* Schur condense / expand on the deterministic step lists (device option schur_deterministic): */
/* the lists of chol_build_solve_det CUT at level k (chol_plan.h at chol_build_schur_det), and  */
/* their host restatement on chunks of 32 columns                                               */
/* ---------------------------------------------------------------------------------------- */
static void schur_det_copy_items(mul_build *b, const chol_sdet_lists *w, int q, const chol_sdet_step *st, int t0, int only_under)
{
  for (int i = st->item_first; i < st->item_end; i++) {
    const chol_mul_item *it = &w->item[q][i];
    int n = 0;
    for (int e = it->src_first; e < it->src_end; e++) n += !only_under || w->src[q][e].z_off < t0;
    if (!n) continue; /* nothing to gather: no item */
    mul_open_item(b, it->y_off, it->nv);
    for (int e = it->src_first; e < it->src_end; e++) {
      const chol_mul_src *s = &w->src[q][e];
      if (only_under && s->z_off >= t0) continue; /* a panel of a kept separator: it holds S, not L */
      mul_push_src(b, s->a_off, s->ld, s->len, s->z_off, s->tri);
    }
    mul_close_item(b);
  }
}
int chol_build_schur_det(const plan_t *p, int k, chol_sdet_lists *out)
{
  memset(out, 0, sizeof *out);
  int t0 = 0;
  const int m = chol_schur_range(p, k, &t0);
  if (m < 0) return m;
  chol_sdet_lists w;
  int rc = chol_build_solve_det(p, &w);
  if (rc) return rc;
  const int n = p->n;
  mul_build b[2] = { { 0 }, { 0 } };
  unsigned char *solved = calloc((size_t)(n > 0 ? n : 1), 1), *owned = calloc((size_t)(n > 0 ? n : 1), 1);
  rc = CHOLAMD_ERR_NOMEM;
  if (!solved || !owned) { chol_set_error("out of memory"); goto done; }
  for (int q = 0; q < 2; q++) {
    out->step[q] = calloc((size_t)w.n_step[q] + 1, sizeof(chol_sdet_step));
    if (!out->step[q]) { chol_set_error("out of memory"); goto done; }
    int t = 0;
    for (int i = 0; i < w.n_step[q]; i++) { /* the steps of the levels under the cut, unchanged and in their order */
      const chol_sdet_step *st = &w.step[q][i];
      if (st->level < k) continue;
      chol_sdet_step *o = &out->step[q][t++];
      o->level = st->level; o->col0 = st->col0; o->item_first = b[q].n_item;
      schur_det_copy_items(&b[q], &w, q, st, t0, 0);
      o->item_end = b[q].n_item;
    }
    if (q == 0) { /* the kept lead step: what the eliminated panels add to the kept positions, one launch */
      chol_sdet_step *o = &out->step[q][t++];
      o->level = -1; o->col0 = -1; o->item_first = b[q].n_item;
      for (int i = 0; i < w.n_step[q]; i++)
        if (w.step[q][i].level < k && w.step[q][i].col0 < 0) schur_det_copy_items(&b[q], &w, q, &w.step[q][i], t0, 1);
      o->item_end = b[q].n_item;
    }
    out->n_step[q] = t;
  }
  for (int q = 0; q < 2; q++) {
    out->item[q] = b[q].item; out->n_item[q] = b[q].n_item; out->src[q] = b[q].src; out->n_src[q] = b[q].n_src;
    b[q].item = NULL; b[q].src = NULL;
  }
  if (b[0].fail || b[1].fail) { chol_set_error("Schur solve lists: out of memory or more than 2^30 sources"); goto done; }
  /* no source may lie in a block of two kept separators.  A source is a strip of ONE panel: FORWARD the panel of the separator its factors z come from,
   * BACKWARD the panel of the separator the item's columns belong to; the panel of a kept separator holds nothing but such blocks */
  rc = CHOLAMD_ERR_INVARIANT;
  for (int q = 0; q < 2; q++)
    for (int i = 0; i < out->n_item[q]; i++) {
      const chol_mul_item *it = &out->item[q][i];
      if (it->nv < 1 || it->nv > CHOL_MUL_TILE || it->y_off < 0 || it->y_off + it->nv > n || it->src_end <= it->src_first) { chol_set_error("internal: Schur solve item %d of direction %d is malformed", i, q); goto done; }
      for (int e = it->src_first; e < it->src_end; e++) {
        const chol_mul_src *s = &out->src[q][e];
        if (s->len < 1 || s->z_off < 0 || s->z_off + s->len > n) { chol_set_error("internal: Schur solve item %d of direction %d: source %d leaves the vector", i, q, e); goto done; }
        const int64_t last = q == 0 ? s->a_off + (it->nv - 1) + (int64_t)(s->len - 1) * s->ld : s->a_off + (s->len - 1) + (int64_t)(it->nv - 1) * s->ld;
        if (s->a_off < 0 || last >= p->arena) { chol_set_error("internal: Schur solve item %d of direction %d: source %d leaves the arena", i, q, e); goto done; }
        if (p->heap_of[p->sep_of_pos[q == 0 ? s->z_off : it->y_off]] < (1 << k)) { chol_set_error("internal: Schur solve item %d of direction %d: source %d lies in a block of two kept separators", i, q, e); goto done; }
      }
    }
  /* the sweeps walked: under the cut every position is solved exactly once and read only after that; the kept positions are read by the expand (they are
   * its input) and owned at most once by the kept lead step, whose sources all lie under the cut */
  for (int q = 0; q < 2; q++) {
    memset(solved, 0, (size_t)(n > 0 ? n : 1));
    memset(owned, 0, (size_t)(n > 0 ? n : 1));
    for (int i = t0; i < n && q == 1; i++) solved[i] = 1; /* xt */
    for (int t = 0; t < out->n_step[q]; t++) {
      const chol_sdet_step *st = &out->step[q][t];
      for (int i = st->item_first; i < st->item_end; i++) {
        const chol_mul_item *it = &out->item[q][i];
        for (int l = 0; l < it->nv; l++) {
          const int pos = it->y_off + l;
          if (st->level < 0) {
            if (pos < t0 || owned[pos]) { chol_set_error("internal: kept lead item %d owns position %d, which lies under the cut or has an owner already", i, pos); goto done; }
            owned[pos] = 1;
          } else if (pos >= t0 || solved[pos]) { chol_set_error("internal: Schur solve item %d of direction %d owns position %d, which is kept or solved already", i, q, pos); goto done; }
        }
        for (int e = it->src_first; e < it->src_end; e++) {
          const chol_mul_src *s = &out->src[q][e];
          if (st->level < 0 && s->z_off + s->len > t0) { chol_set_error("internal: kept lead item %d: source %d reads position %d at or above the cut", i, e, s->z_off + s->len - 1); goto done; }
          for (int c = 0; c < s->len; c++)
            if (!solved[s->z_off + c]) { chol_set_error("internal: Schur solve item %d of direction %d: source %d reads position %d before it is solved", i, q, e, s->z_off + c); goto done; }
        }
      }
      if (st->col0 < 0) continue;
      for (int h = 1 << st->level; h < (1 << (st->level + 1)) && h <= p->nsep; h++) {
        const int s = p->tree[h];
        for (int i = st->col0; i < p->sep_size[s] && i < st->col0 + CHOL_SDET_SPAN; i++) {
          const int pos = p->sep_off[s] + i;
          if (pos >= t0 || solved[pos]) { chol_set_error("internal: Schur sweep %d solves position %d twice or above the cut", q, pos); goto done; }
          solved[pos] = 1;
        }
      }
    }
    for (int i = 0; i < t0; i++) if (!solved[i]) { chol_set_error("internal: Schur sweep %d never solves position %d", q, i); goto done; }
  }
  rc = 0;
done:
  free(solved); free(owned);
  for (int q = 0; q < 2; q++) { free(b[q].item); free(b[q].src); }
  chol_sdet_lists_free(&w);
  if (rc) chol_sdet_lists_free(out);
  return rc;
}
/* one sweep of the cut lists on the permuted row-major block: sdet_host_block_sweep's arithmetic (the kernel's partition of a gather, substitution inside a
 * span's own triangle); a kept lead step (level -1) has no span */
static void schur_det_host_block_sweep(const plan_t *p, const chol_sdet_lists *w, int which, const double *arena, double *yp)
{
  chol_sdet_lists one = *w; /* a step at a time through the walk of the whole-tree lists; the kept lead step has col0 < 0, so its level is never looked at */
  for (int t = 0; t < w->n_step[which]; t++) {
    one.n_step[which] = 1; one.step[which] = (chol_sdet_step *)&w->step[which][t];
    sdet_host_block_sweep(p, &one, which, arena, yp);
  }
}
static int schur_nrhs_host_args(const plan_t *p, int k, const char *what, const void *arena, const void *a, const void *b, const void *c, const char *na, const char *nb, const char *nc,
                                int64_t lda, int64_t ldb, int64_t ldc, int rows_a, int rows_b, int rows_c, int nrhs)
{ /* 1: nothing to do */
  if (nrhs < 0) { chol_set_error("%s: nrhs = %d < 0", what, nrhs); return CHOLAMD_ERR_ARG; }
  if (lda < rows_a || ldb < rows_b || ldc < rows_c) {
    chol_set_error("%s: leading dimensions of %s, %s, %s = %lld, %lld, %lld must be at least %d, %d, %d", what, na, nb, nc, (long long)lda, (long long)ldb, (long long)ldc, rows_a, rows_b, rows_c);
    return CHOLAMD_ERR_ARG;
  }
  if (nrhs == 0) return 1;
  if (!arena || !a || !b || !c) { chol_set_error("%s: NULL %s", what, !arena ? "arena" : !a ? na : !b ? nb : nc); return CHOLAMD_ERR_ARG; }
  (void)p; (void)k;
  return 0;
}
int cholamd_plan_schur_condense_host_nrhs(const cholamd_plan *p, int k, const double *arena_host, const double *B, int64_t ldb, double *W, int64_t ldw, double *G, int64_t ldg, int nrhs)
{
  const char *what = "cholamd_plan_schur_condense_host_nrhs";
  if (!p) { chol_set_error("%s: NULL plan", what); return CHOLAMD_ERR_ARG; }
  int t0 = 0;
  const int m = chol_schur_range(p, k, &t0), n = p->n;
  if (m < 0) return m;
  { int rc = schur_nrhs_host_args(p, k, what, arena_host, B, W, G, "B", "W", "G", ldb, ldw, ldg, n, n, m, nrhs); if (rc) return rc > 0 ? 0 : rc; }
  chol_sdet_lists w;
  int rc = chol_build_schur_det(p, k, &w);
  if (rc) return rc;
  double *yp = malloc((size_t)(n > 0 ? n : 1) * 32 * sizeof(double));
  if (!yp) { chol_sdet_lists_free(&w); chol_set_error("out of memory"); return CHOLAMD_ERR_NOMEM; }
  for (int c0 = 0; c0 < nrhs; c0 += 32) {
    const int cols = nrhs - c0 < 32 ? nrhs - c0 : 32;
    for (int i = 0; i < n; i++)
      for (int j = 0; j < 32; j++) yp[(int64_t)i * 32 + j] = j < cols ? B[p->perm[i] + (int64_t)(c0 + j) * ldb] : 0.0;
    schur_det_host_block_sweep(p, &w, CHOLAMD_HALF_FORWARD, arena_host, yp);
    for (int i = 0; i < n; i++)
      for (int j = 0; j < cols; j++) {
        W[i + (int64_t)(c0 + j) * ldw] = yp[(int64_t)i * 32 + j];
        if (i >= t0) G[(i - t0) + (int64_t)(c0 + j) * ldg] = yp[(int64_t)i * 32 + j];
      }
  }
  free(yp);
  chol_sdet_lists_free(&w);
  return 0;
}
int cholamd_plan_schur_expand_host_nrhs(const cholamd_plan *p, int k, const double *arena_host, const double *W, int64_t ldw, const double *XT, int64_t ldxt, double *X, int64_t ldx, int nrhs)
{
  const char *what = "cholamd_plan_schur_expand_host_nrhs";
  if (!p) { chol_set_error("%s: NULL plan", what); return CHOLAMD_ERR_ARG; }
  int t0 = 0;
  const int m = chol_schur_range(p, k, &t0), n = p->n;
  if (m < 0) return m;
  { int rc = schur_nrhs_host_args(p, k, what, arena_host, W, XT, X, "W", "XT", "X", ldw, ldxt, ldx, n, m, n, nrhs); if (rc) return rc > 0 ? 0 : rc; }
  chol_sdet_lists w;
  int rc = chol_build_schur_det(p, k, &w);
  if (rc) return rc;
  double *yp = malloc((size_t)(n > 0 ? n : 1) * 32 * sizeof(double));
  if (!yp) { chol_sdet_lists_free(&w); chol_set_error("out of memory"); return CHOLAMD_ERR_NOMEM; }
  for (int c0 = 0; c0 < nrhs; c0 += 32) {
    const int cols = nrhs - c0 < 32 ? nrhs - c0 : 32;
    for (int i = 0; i < n; i++)
      for (int j = 0; j < 32; j++)
        yp[(int64_t)i * 32 + j] = j >= cols ? 0.0 : i < t0 ? W[i + (int64_t)(c0 + j) * ldw] : XT[(i - t0) + (int64_t)(c0 + j) * ldxt];
    schur_det_host_block_sweep(p, &w, CHOLAMD_HALF_BACKWARD, arena_host, yp);
    for (int i = 0; i < n; i++)
      for (int j = 0; j < cols; j++) X[p->perm[i] + (int64_t)(c0 + j) * ldx] = yp[(int64_t)i * 32 + j];
  }
  free(yp);
  chol_sdet_lists_free(&w);
  return 0;
}
int cholamd_plan_schur_det_counts(const cholamd_plan *p, int k, int64_t out[8])
{
  if (!p || !out) { chol_set_error("cholamd_plan_schur_det_counts: NULL %s", !p ? "plan" : "out"); return CHOLAMD_ERR_ARG; }
  chol_sdet_lists w;
  int rc = chol_build_schur_det(p, k, &w);
  if (rc) return rc;
  for (int d = 0; d < 2; d++) {
    int64_t entries = 0;
    for (int i = 0; i < w.n_item[d]; i++)
      for (int e = w.item[d][i].src_first; e < w.item[d][i].src_end; e++) entries += (int64_t)w.item[d][i].nv * w.src[d][e].len;
    for (int h = 1 << k; h <= p->nsep; h++) /* the spans' own lower triangles, under the cut */
      for (int c0 = 0; c0 < p->sep_size[p->tree[h]]; c0 += CHOL_SDET_SPAN) {
        const int64_t mm = p->sep_size[p->tree[h]] - c0 < CHOL_SDET_SPAN ? p->sep_size[p->tree[h]] - c0 : CHOL_SDET_SPAN;
        entries += mm * (mm + 1) / 2;
      }
    out[4 * d] = w.n_step[d]; out[4 * d + 1] = w.n_item[d]; out[4 * d + 2] = w.n_src[d]; out[4 * d + 3] = entries;
  }
  chol_sdet_lists_free(&w);
  return 0;
}
int cholamd_plan_schur_det_lists(const cholamd_plan *p, int k, int which, int64_t *steps, int64_t *items, int64_t *srcs)
{
  if (!p || !steps || !items || !srcs) { chol_set_error("cholamd_plan_schur_det_lists: NULL %s", !p ? "plan" : "output"); return CHOLAMD_ERR_ARG; }
  if (which != CHOLAMD_HALF_FORWARD && which != CHOLAMD_HALF_BACKWARD) { chol_set_error("cholamd_plan_schur_det_lists: which = %d is neither CHOLAMD_HALF_FORWARD (0) nor CHOLAMD_HALF_BACKWARD (1)", which); return CHOLAMD_ERR_ARG; }
  chol_sdet_lists w;
  int rc = chol_build_schur_det(p, k, &w);
  if (rc) return rc;
  for (int t = 0; t < w.n_step[which]; t++) {
    const chol_sdet_step *s = &w.step[which][t];
    steps[4 * t] = s->level; steps[4 * t + 1] = s->col0; steps[4 * t + 2] = s->item_first; steps[4 * t + 3] = s->item_end;
  }
  for (int i = 0; i < w.n_item[which]; i++) {
    const chol_mul_item *it = &w.item[which][i];
    items[4 * i] = it->y_off; items[4 * i + 1] = it->nv; items[4 * i + 2] = it->src_first; items[4 * i + 3] = it->src_end;
  }
  for (int e = 0; e < w.n_src[which]; e++) {
    const chol_mul_src *q = &w.src[which][e];
    srcs[5 * e] = q->a_off; srcs[5 * e + 1] = q->ld; srcs[5 * e + 2] = q->len; srcs[5 * e + 3] = q->z_off; srcs[5 * e + 4] = q->tri;
  }
  chol_sdet_lists_free(&w);
  return 0;
}
