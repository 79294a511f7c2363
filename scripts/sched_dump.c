/* Development aid: are the lists of the two schedule builders the same in two builds?  Prints, for a fixed set of inputs, option sets and
 * (level, rank, world), one line per array chol_build_level_work / chol_build_program emit: element count and a 64-bit FNV-1a hash over the
 * fields in array order (field by field: padding bytes are undefined).  A refused build prints its return code and cholamd_last_error().
 * Build it in both trees against the six host objects (no HIP), run both from the repository root and diff:
 *   gcc -O2 -std=gnu11 -Iinclude -Icholesky_amd/csrc scripts/sched_dump.c cholesky_amd/lib/chol_{ingest,symbolic,schedule,lists,generate,lowrank_host}.o -lm -o sched_dump
 *   ./sched_dump tests/golden > dump.txt          the whole set
 *   ./sched_dump tests/golden --grid 30,30,30,4,16   one more generated grid (nx,ny,nz,levels,tile) after the built-in ones
 *   ./sched_dump tests/golden --only-grid ...     that grid alone (trying sizes)
 *   ./sched_dump tests/golden --digest            the same walk, one line per (input, option set): lines of the full dump and their hash
 *   ./sched_dump tests/golden --time              program + every level's lists of lapl_3375x3375 at the defaults, 30 times: min median max (us)
 * Field names only, so that it compiles against trees before and after a change of the builders' internals. */
#define _GNU_SOURCE
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "chol_plan.h"
#include "cholamd.h"

static uint64_t fnv(uint64_t h, const void *v, size_t n)
{
  const unsigned char *b = v;
  for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}
#define FNV0 14695981039346656037ull
#define H(x) h = fnv(h, &(x), sizeof(x))
/* every line of the dump goes through out(): printed, or (--digest) folded into the hash of its section */
static int digest;
static uint64_t dg_hash = FNV0;
static long dg_lines;
static char dg_name[256];
static void out(const char *fmt, ...)
{
  char buf[1400];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (!digest) { fputs(buf, stdout); return; }
  dg_hash = fnv(dg_hash, buf, strlen(buf));
  dg_lines++;
}
static void section(const char *input, const char *options)
{
  if (digest && dg_lines) printf("%s: %ld lines %016llx\n", dg_name, dg_lines, (unsigned long long)dg_hash);
  dg_hash = FNV0; dg_lines = 0;
  if (input) snprintf(dg_name, sizeof dg_name, "%s, %s", input, options);
}
#define LINE(name, n) out("    %-9s %8d %016llx\n", name, (int)(n), (unsigned long long)h)

static void dump_work(const chol_level_work *w)
{
  uint64_t h = FNV0;
  for (int i = 0; i < w->n_phase; i++) { const chol_phase *x = &w->phase[i]; H(x->kind); H(x->first); H(x->n); H(x->first2); H(x->n2); H(x->first3); H(x->n3); }
  LINE("phase", w->n_phase);
  h = FNV0;
  for (int i = 0; i < w->n_potrf; i++) { const chol_potrf_desc *x = &w->potrf[i]; H(x->a_off); H(x->dinv_off); H(x->n); H(x->lda); H(x->sep); H(x->col0); H(x->ctr); H(x->tab); H(x->sky); }
  LINE("potrf", w->n_potrf);
  h = FNV0;
  for (int i = 0; i < w->n_trsm; i++) { const chol_trsm_desc *x = &w->trsm[i]; H(x->l_off); H(x->dinv_off); H(x->b_off); H(x->n); H(x->ldl); H(x->m); H(x->ldb); H(x->flag); H(x->chan); H(x->band); H(x->pad); }
  LINE("trsm", w->n_trsm);
  for (int pass = 0; pass < 2; pass++) {
    const chol_upd_task *T = pass ? w->task_mt : w->task;
    const int nt = pass ? w->n_task_mt : w->n_task;
    h = FNV0;
    for (int i = 0; i < nt; i++) { const chol_upd_task *x = &T[i]; H(x->c_off); H(x->ldc); H(x->mv); H(x->nv); H(x->lower); H(x->src_begin); H(x->src_end); H(x->ar); H(x->br); H(x->blk); }
    LINE(pass ? "task_mt" : "task", nt);
  }
  h = FNV0;
  for (int i = 0; i < w->n_src; i++) { const chol_upd_src *x = &w->src[i]; H(x->a_off); H(x->b_off); H(x->lda); H(x->ldb); H(x->k); H(x->range); H(x->stage); H(x->pad); }
  LINE("src", w->n_src);
  h = FNV0;
  for (int i = 0; i < w->n_bcast; i++) { const chol_bcast *x = &w->bcast[i]; H(x->off); H(x->count); H(x->owner); H(x->heap); }
  LINE("bcast", w->n_bcast);
}
static void dump_program(const chol_program *g)
{
  uint64_t h = FNV0;
  for (int i = 0; i < g->n_job; i++) { const chol_job *x = &g->job[i]; H(x->kind); H(x->first); H(x->n); H(x->wait_first); H(x->n_wait); H(x->sig[0]); H(x->sig[1]); H(x->sig_add); H(x->ext_first); H(x->n_ext); H(x->mode); H(x->n_pre); }
  LINE("job", g->n_job);
  h = FNV0;
  for (int i = 0; i < g->n_wait; i++) { H(g->wait[i].ctr); H(g->wait[i].value); }
  LINE("wait", g->n_wait);
  h = FNV0;
  for (int i = 0; i < g->n_ext; i++) { const chol_ext *x = &g->ext[i]; H(x->off); H(x->ld); H(x->ncol); H(x->ctr); H(x->need); }
  LINE("ext", g->n_ext);
  h = FNV0;
  for (int i = 0; i < g->n_ctr; i++) H(g->ctr_total[i]);
  LINE("ctr_total", g->n_ctr);
  h = FNV0; H(g->follow);
  LINE("follow", 1);
}

/* an option set: up to four (field, value) settings against the defaults; env: CHOLAMD_NO_LEAF_ORDER is set; dist: also run at worlds 2, 4, 8 */
typedef struct { const char *name; struct { size_t off; int v; } set[5]; int nset, env, dist; } opt_set;
#define F(f) offsetof(chol_sched_opts, f)
static const opt_set SETS[] = {
  { "defaults", { { 0, 0 } }, 0, 0, 1 },
  { "follow=0", { { F(follow), 0 } }, 1, 0, 0 },
  { "cells=0", { { F(cells), 0 } }, 1, 0, 1 },
  { "fuse=0", { { F(fuse), 0 } }, 1, 0, 1 },
  { "follow_tail=0", { { F(follow_tail), 0 } }, 1, 0, 0 },
  { "follow_tail=1", { { F(follow_tail), 1 } }, 1, 0, 0 },
  { "follow_tail=2", { { F(follow_tail), 2 } }, 1, 0, 0 },
  { "follow_tail=4", { { F(follow_tail), 4 } }, 1, 0, 0 },
  { "follow_tail=6", { { F(follow_tail), 6 } }, 1, 0, 0 },
  { "follow_tail_split=0", { { F(follow_tail_split), 0 } }, 1, 0, 0 },
  { "follow_tail_split=2", { { F(follow_tail_split), 2 } }, 1, 0, 0 },
  { "follow_own=0", { { F(follow_own), 0 } }, 1, 0, 0 },
  { "follow_own=1", { { F(follow_own), 1 } }, 1, 0, 0 },
  { "follow_own=2", { { F(follow_own), 2 } }, 1, 0, 0 },
  { "split=64/64", { { F(split_min), 64 }, { F(split_nb), 64 } }, 2, 0, 1 },
  { "split=96/96", { { F(split_min), 96 }, { F(split_nb), 96 } }, 2, 0, 0 },
  { "split=32/32", { { F(split_min), 32 }, { F(split_nb), 32 } }, 2, 0, 0 },
  { "split=16/16", { { F(split_min), 16 }, { F(split_nb), 16 } }, 2, 0, 0 },
  { "split=192/192", { { F(split_min), 192 }, { F(split_nb), 192 } }, 2, 0, 0 },
  { "split=64/64,follow_tail_split=2,follow_own=2", { { F(split_min), 64 }, { F(split_nb), 64 }, { F(follow_tail_split), 2 }, { F(follow_own), 2 } }, 4, 0, 0 },
  { "skyline=0", { { F(skyline), 0 } }, 1, 0, 0 },
  { "stage_chunk=2", { { F(stage_chunk), 2 } }, 1, 0, 0 },
  { "stage_chunk=4", { { F(stage_chunk), 4 } }, 1, 0, 0 },
  { "staged=0", { { F(staged), 0 } }, 1, 0, 0 },
  { "fine_upd=0", { { F(fine_upd), 0 } }, 1, 0, 0 },
  { "merge_targets=0", { { F(merge_targets), 0 } }, 1, 0, 1 },
  { "leaf_envelope=0", { { F(leaf_envelope), 0 } }, 1, 0, 0 },
  { "mt_min_tiles=1", { { F(mt_min_tiles), 1 } }, 1, 0, 1 },
  { "trsm_wt_min=0", { { F(trsm_wt_min), 0 } }, 1, 0, 0 },
  { "trsm_wt_min=1", { { F(trsm_wt_min), 1 } }, 1, 0, 1 },
  { "super_blocks=1", { { F(super_blocks), 1 } }, 1, 0, 0 },
  { "super_blocks=2", { { F(super_blocks), 2 } }, 1, 0, 0 },
  { "fuse_update_max=64", { { F(fuse_update_max), 64 } }, 1, 0, 0 },
  { "fuse_update_max=1<<30", { { F(fuse_update_max), 1 << 30 } }, 1, 0, 0 },
  { "fp32", { { F(split_min), CHOL32_MAXN }, { F(split_nb), CHOL32_MAXN }, { F(fuse), 0 }, { F(fuse_update_max), 0 }, { F(trsm_group), CHOL32_TRSM_GROUP } }, 5, 0, 1 },
  { "CHOLAMD_NO_LEAF_ORDER", { { 0, 0 } }, 0, 1, 0 },
};
#undef F

static void run_levels(const cholamd_plan *p, const chol_sched_opts *o, int rank, int world)
{
  for (int level = p->levels - 1; level >= 0; level--) {
    chol_level_work w;
    const int rc = chol_build_level_work(p, o, level, rank, world, &w);
    out("  level %d rank %d world %d dist_top %d\n", level, rank, world, o->dist_top);
    if (rc) { out("    refused %d: %s\n", rc, cholamd_last_error()); continue; }
    dump_work(&w);
    chol_level_work_free(&w);
  }
}
static void run_plan(const cholamd_plan *p, const char *name)
{
  int64_t leaf_rows = 0;
  for (int h = 1 << (p->levels - 1); h <= p->nsep; h++) leaf_rows += p->panel_rows[p->tree[h]];
  printf("input %s: n %d levels %d leaf panel rows %lld\n", name, p->n, p->levels, (long long)leaf_rows);
  for (size_t k = 0; k < sizeof SETS / sizeof SETS[0]; k++) {
    const opt_set *s = &SETS[k];
    chol_sched_opts o;
    chol_sched_opts_default(&o);
    for (int i = 0; i < s->nset; i++) *(int *)((char *)&o + s->set[i].off) = s->set[i].v;
    if (s->env) setenv("CHOLAMD_NO_LEAF_ORDER", "1", 1); else unsetenv("CHOLAMD_NO_LEAF_ORDER");
    section(name, s->name);
    out(" options %s\n", s->name);
    run_levels(p, &o, 0, 1);
    chol_level_work w; chol_program g;
    const int rc = chol_build_program(p, &o, &w, &g);
    out("  program\n");
    if (rc) out("    refused %d: %s\n", rc, cholamd_last_error());
    else { dump_work(&w); dump_program(&g); chol_level_work_free(&w); chol_program_free(&g); }
    if (!s->dist) continue;
    for (int world = 2; world <= 8; world *= 2)
      for (int rank = 0; rank < world; rank++)
        for (o.dist_top = 0; o.dist_top <= 2; o.dist_top++) run_levels(p, &o, rank, world);
  }
  section(NULL, NULL);
  unsetenv("CHOLAMD_NO_LEAF_ORDER");
}
static int run_grid(int nx, int ny, int nz, int levels, int tile)
{
  char name[96];
  snprintf(name, sizeof name, "gen(%d,%d,%d,%d,%d)", nx, ny, nz, levels, tile);
  cholamd_problem *g = NULL;
  cholamd_plan *p = NULL;
  if (cholamd_generate_laplacian(nx, ny, nz, levels, tile, &g) || cholamd_plan_create_from_problem(g, &p)) { fprintf(stderr, "%s: %s\n", name, cholamd_last_error()); return 1; }
  run_plan(p, name);
  cholamd_plan_destroy(p);
  cholamd_problem_destroy(g);
  return 0;
}
static int fixture_plan(const char *golden, const char *dir, const char *stem, int lv, cholamd_plan **out)
{
  char a[512], b[512], c[512];
  snprintf(a, sizeof a, "%s/%s/%s.mtx", golden, dir, stem);
  snprintf(b, sizeof b, "%s/%s/%s_ord_%d.txt", golden, dir, stem, lv);
  snprintf(c, sizeof c, "%s/%s/%s_clust_%d.txt", golden, dir, stem, lv);
  if (cholamd_plan_create(a, b, c, out)) { fprintf(stderr, "%s: %s\n", a, cholamd_last_error()); return 1; }
  return 0;
}
static int cmp_double(const void *x, const void *y) { const double a = *(const double *)x, b = *(const double *)y; return a < b ? -1 : a > b; }
static int run_time(const char *golden)
{
  cholamd_plan *p = NULL;
  if (fixture_plan(golden, "lapl_3375x3375", "lapl_15_3", 5, &p)) return 1;
  double us[30];
  for (int r = 0; r < 30; r++) {
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    chol_level_work w; chol_program g;
    if (chol_build_program(p, NULL, &w, &g)) return 1;
    chol_level_work_free(&w); chol_program_free(&g);
    for (int level = p->levels - 1; level >= 0; level--) {
      if (chol_build_level_work(p, NULL, level, 0, 1, &w)) return 1;
      chol_level_work_free(&w);
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    us[r] = (t1.tv_sec - t0.tv_sec) * 1e6 + (t1.tv_nsec - t0.tv_nsec) * 1e-3;
  }
  qsort(us, 30, sizeof(double), cmp_double);
  printf("lists of lapl_3375x3375, 30 builds: min %.1f median %.1f max %.1f us\n", us[0], 0.5 * (us[14] + us[15]), us[29]);
  cholamd_plan_destroy(p);
  return 0;
}

int main(int argc, char **argv)
{
  if (argc < 2) { fprintf(stderr, "usage: sched_dump tests/golden [--time | --digest | --grid nx,ny,nz,levels,tile ... | --only-grid nx,ny,nz,levels,tile]\n"); return 2; }
  if (argc > 2 && !strcmp(argv[2], "--time")) return run_time(argv[1]);
  if (argc > 2 && !strcmp(argv[2], "--digest")) { digest = 1; for (int a = 2; a + 1 < argc; a++) argv[a] = argv[a + 1]; argc--; }
  int g[5];
  if (argc > 3 && !strcmp(argv[2], "--only-grid")) {
    if (sscanf(argv[3], "%d,%d,%d,%d,%d", &g[0], &g[1], &g[2], &g[3], &g[4]) != 5) return 2;
    return run_grid(g[0], g[1], g[2], g[3], g[4]);
  }
  static const struct { const char *dir, *stem; int lv; } FIX[4] = { { "lapl_9x9", "lapl_3_2", 2 }, { "lapl_25x25", "lapl_5_2", 3 }, { "lapl_400x400", "lapl_20_2", 5 }, { "lapl_3375x3375", "lapl_15_3", 5 } };
  for (int i = 0; i < 4; i++) {
    cholamd_plan *p = NULL;
    if (fixture_plan(argv[1], FIX[i].dir, FIX[i].stem, FIX[i].lv, &p)) return 1;
    run_plan(p, FIX[i].dir);
    cholamd_plan_destroy(p);
  }
  /* (24,24,12,2,64): the program refuses it; (39,39,39,4,16): the smallest cube at these levels / tile whose leaf level has 65536 panel rows (64-row leaf pieces) */
  static const int GRID[6][5] = { { 7, 5, 3, 3, 4 }, { 12, 12, 12, 4, 16 }, { 10, 9, 8, 5, 8 }, { 14, 14, 14, 4, 16 }, { 24, 24, 12, 2, 64 }, { 39, 39, 39, 4, 16 } };
  for (int i = 0; i < 6; i++) if (run_grid(GRID[i][0], GRID[i][1], GRID[i][2], GRID[i][3], GRID[i][4])) return 1;
  for (int a = 2; a + 1 < argc; a += 2) {
    if (strcmp(argv[a], "--grid") || sscanf(argv[a + 1], "%d,%d,%d,%d,%d", &g[0], &g[1], &g[2], &g[3], &g[4]) != 5) return 2;
    if (run_grid(g[0], g[1], g[2], g[3], g[4])) return 1;
  }
  return 0;
}
