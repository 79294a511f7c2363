// C ABI glue of libcholamd, the task-level (fused_*) and the BLAS-level entry points: per-call scratch, the stand-alone batched launches, regions and
// fused leaf tasks, the debug driver, the device-pointer BLAS and the host-pointer CBLAS / LAPACKE replacements.  Compiled with hipcc like chol_api.cpp.
#include "chol_device.h"

// ---------------------------------------------------------------------------------------------
// L-A / L-B: stand-alone batched launches with pointer-valued descriptors (base = nullptr)
// ---------------------------------------------------------------------------------------------
static inline int64_t poff(const void *p) { return (int64_t)((uintptr_t)p / sizeof(double)); }

struct scratch { // per-call device scratch, freed at scope exit after the stream has been synchronised
  std::vector<dev_buf<char>> bufs;
  template <class T> int get(T **dptr, size_t n, int floating_point = std::is_floating_point<T>::value)
  {
    bufs.emplace_back();
    int rc = bufs.back().alloc_bytes((n ? n : 1) * sizeof(T), floating_point);
    *dptr = (T *)bufs.back().get();
    return rc;
  }
  template <class T> int put(T **dptr, const T *h, size_t n, hipStream_t st)
  {
    *dptr = nullptr;
    if (n == 0) return 0;
    int rc = get(dptr, n, 0); // uploads: plain memory
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(*dptr, h, n * sizeof(T), hipMemcpyHostToDevice, st));
    return 0;
  }
};

static int check_ptr(const void *p, const char *what)
{
  if (!p || ((uintptr_t)p & 7)) { chol_set_error("%s must be a non-null, 8-byte aligned pointer", what); return CHOLAMD_ERR_ARG; }
  return 0;
}
static int have_device()
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return no_device_error();
  return 0;
}

static void add_update_tasks(std::vector<chol_upd_task> &tasks, int src_begin, int src_end, double *c, int ldc, int m, int n, bool syrk)
{
  const int tr = (m + 15) / 16, tc = (n + 15) / 16;
  for (int a = 0; a < tr; a++)
    for (int b = 0; b < tc; b++) {
      if (syrk && b > a) continue;
      chol_upd_task t;
      std::memset(&t, 0, sizeof t);
      t.c_off = poff(c) + a * 16 + (int64_t)b * 16 * ldc;
      t.ldc = ldc;
      t.mv = (short)(m - a * 16 < 16 ? m - a * 16 : 16);
      t.nv = (short)(n - b * 16 < 16 ? n - b * 16 : 16);
      t.lower = (syrk && a == b);
      t.src_begin = src_begin; t.src_end = src_end; t.ar = a * 16; t.br = b * 16;
      tasks.push_back(t);
    }
}

static int run_updates(std::vector<chol_upd_task> &tasks, std::vector<chol_upd_src> &srcs, hipStream_t st)
{
  if (tasks.empty()) return 0;
  scratch sc;
  chol_upd_task *dt; chol_upd_src *ds;
  int rc = sc.put(&dt, tasks.data(), tasks.size(), st);
  if (!rc) rc = sc.put(&ds, srcs.data(), srcs.size(), st);
  if (rc) return rc;
  HIPCHK((hipError_t)chol_launch_update((double *)nullptr, dt, ds, (int)tasks.size(), st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// B tiles (rows m_i of width n) <- B L^-T for one pivot L (n x n, ld ldl)
static int run_trsm(const double *Lp, int n, int ldl, const std::vector<chol_trsm_desc> &rows, hipStream_t st)
{
  if (rows.empty() || n == 0) return 0;
  scratch sc;
  double *W; chol_trsm_desc *dd;
  const size_t nb = (size_t)(n + CHOL_NB - 1) / CHOL_NB;
  int rc = sc.get(&W, nb * CHOL_NB * CHOL_NB);
  if (rc) return rc;
  HIPCHK((hipError_t)chol_launch_dinv(Lp, n, ldl, W, st));
  std::vector<chol_trsm_desc> v;
  for (const auto &r : rows)
    for (int r0 = 0; r0 < r.m; r0 += CHOL_TRSM_ROWS) {
      chol_trsm_desc t = r;
      t.l_off = poff(Lp); t.dinv_off = poff(W); t.b_off = r.b_off + r0;
      t.m = r.m - r0 < CHOL_TRSM_ROWS ? r.m - r0 : CHOL_TRSM_ROWS;
      v.push_back(t);
    }
  rc = sc.put(&dd, v.data(), v.size(), st);
  if (rc) return rc;
  if (n <= CHOL_TRSM_W_MAXN) HIPCHK((hipError_t)chol_launch_trsm_w(nullptr, nullptr, dd, (int)v.size(), st));
  else if (n <= CHOL_RR_MAXN) HIPCHK((hipError_t)chol_launch_trsm((double *)nullptr, nullptr, dd, (int)v.size(), st));
  else HIPCHK((hipError_t)chol_launch_trsm_big(nullptr, nullptr, dd, (int)v.size(), st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

static int run_potrf(const std::vector<chol_potrf_desc> &v, hipStream_t st, int *info_out, int *sep_out)
{
  if (info_out) *info_out = 0;
  if (v.empty()) return 0;
  scratch sc;
  size_t wsz = 0;
  std::vector<chol_potrf_desc> dv;
  for (const auto &p : v) if (p.n <= CHOL_RR_MAXN) dv.push_back(p);
  const int n_small = (int)dv.size();
  for (const auto &p : v) if (p.n > CHOL_RR_MAXN) dv.push_back(p);
  for (auto &p : dv) { p.dinv_off = (int64_t)wsz; wsz += (size_t)((p.n + CHOL_NB - 1) / CHOL_NB) * CHOL_NB * CHOL_NB; }
  double *W; int *info; chol_potrf_desc *dd;
  int rc = sc.get(&W, wsz);
  if (!rc) rc = sc.get(&info, (size_t)2);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(info, 0, 2 * sizeof(int), st));
  rc = sc.put(&dd, dv.data(), dv.size(), st);
  if (rc) return rc;
  HIPCHK((hipError_t)chol_launch_potrf(nullptr, W, dd, n_small, info, st));
  HIPCHK((hipError_t)chol_launch_potrf_big(nullptr, W, dd + n_small, (int)dv.size() - n_small, info, st));
  int h[2] = { 0, 0 };
  HIPCHK(hipMemcpyAsync(h, info, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (info_out) *info_out = h[0];
  if (sep_out) *sep_out = h[1];
  return 0;
}

// ---- L-B: fused leaf tasks -------------------------------------------------------------------
static double *tile_ptr(const cholamd_region *r, const cholamd_filled *f)
{ // get_raw_ptr_2d, blas.rg:35-43; a row-compacted block instance stores only the 16-row tiles its filled tiles touch (tile_row)
  const int row = f->lo_x - r->lo_x;
  const int64_t srow = r->tile_row ? (int64_t)r->tile_row[row / CHOL_NB] * CHOL_NB + row % CHOL_NB : row;
  return r->ptr + srow + (int64_t)(f->lo_y - r->lo_y) * r->ld;
}
static int region_ok(const cholamd_region *r, const char *name)
{
  if (!r) { chol_set_error("region %s is null", name); return CHOLAMD_ERR_ARG; }
  return check_ptr(r->ptr, name);
}
static int tile_inside(const cholamd_region *r, const cholamd_filled *f)
{
  if (f->lo_x < r->lo_x || f->lo_y < r->lo_y || f->hi_x > r->hi_x || f->hi_y > r->hi_y) {
    chol_set_error("tile (%d,%d,%d) lies outside its region", f->sep_x, f->sep_y, f->cluster);
    return CHOLAMD_ERR_ARG;
  }
  if (r->tile_row) // every row of the tile must have storage, consecutively
    for (int t = (f->lo_x - r->lo_x) / CHOL_NB; t <= (f->hi_x - r->lo_x) / CHOL_NB; t++)
      if (r->tile_row[t] < 0 || (t > (f->lo_x - r->lo_x) / CHOL_NB && r->tile_row[t] != r->tile_row[t - 1] + 1)) {
        chol_set_error("tile (%d,%d,%d) touches rows its region does not store", f->sep_x, f->sep_y, f->cluster);
        return CHOLAMD_ERR_ARG;
      }
  return 0;
}

extern "C" int cholamd_plan_region(const cholamd_plan *p, double *d_arena, int r, int c, cholamd_region *out)
{
  const chol_block *B = chol_plan_block(p, r, c);
  if (!B || !out) { chol_set_error("no block (%d, %d)", r, c); return CHOLAMD_ERR_ARG; }
  cholamd_region rg = { d_arena + B->off, B->ld, B->lo_x, B->lo_y, B->hi_x, B->hi_y, B->tmap };
  *out = rg;
  return 0;
}

extern "C" int cholamd_fused_dpotrf(const cholamd_region *rA, const cholamd_filled *fa, int nA, int level, int interval, int debug, void *stream)
{
  int rc = have_device();
  if (!rc) rc = region_ok(rA, "rA");
  if (rc) return rc;
  std::vector<chol_potrf_desc> v;
  for (int i = 0; i < nA; i++) {
    if ((rc = tile_inside(rA, &fa[i]))) return rc;
    const int m = fa[i].hi_x - fa[i].lo_x + 1;
    if (debug)
      printf("POTRF: {'A': (%d, %d, %d), 'A_Lo': (%d, %d), 'A_Hi': (%d, %d), 'SizeA': (%d, %d), 'Block': (%d, %d), 'Level': %d, 'Interval': %d}\n",
             fa[i].sep_x, fa[i].sep_y, fa[i].cluster, fa[i].lo_x, fa[i].lo_y, fa[i].hi_x, fa[i].hi_y, m, fa[i].hi_y - fa[i].lo_y + 1,
             fa[i].sep_x, fa[i].sep_y, level, interval);
    if (m == 0) continue; // blas.rg:68
    chol_potrf_desc p = { poff(tile_ptr(rA, &fa[i])), 0, m, rA->ld, fa[i].sep_x, 0, 0, 0, { 0 } };
    v.push_back(p);
  }
  int info = 0;
  rc = run_potrf(v, (hipStream_t)stream, &info, nullptr);
  return rc ? rc : info;
}

extern "C" int cholamd_fused_dtrsm(const cholamd_region *rA, const cholamd_region *rB, const cholamd_filled *fa, int nA,
                                   const cholamd_filled *fb, int nB, int level, int interval, int debug, void *stream)
{
  int rc = have_device();
  if (!rc) rc = region_ok(rA, "rA");
  if (!rc) rc = region_ok(rB, "rB");
  if (rc) return rc;
  for (int i = 0; i < nA; i++) {
    if ((rc = tile_inside(rA, &fa[i]))) return rc;
    const double *Lp = tile_ptr(rA, &fa[i]);
    std::vector<chol_trsm_desc> rows;
    int n = 0;
    for (int j = 0; j < nB; j++) {
      if ((rc = tile_inside(rB, &fb[j]))) return rc;
      const int m = fb[j].hi_x - fb[j].lo_x + 1;
      n = fb[j].hi_y - fb[j].lo_y + 1;
      if (debug)
        printf("TRSM: {'A': (%d, %d, %d), 'A_Lo': (%d, %d), 'A_Hi': (%d, %d), 'SizeA': (%d, %d), 'B': (%d, %d, %d), 'B_Lo': (%d, %d), 'B_Hi': (%d, %d), 'SizeB': (%d, %d), 'Block': (%d, %d), 'Level': %d, 'Interval': %d}\n",
               fa[i].sep_x, fa[i].sep_y, fa[i].cluster, fa[i].lo_x, fa[i].lo_y, fa[i].hi_x, fa[i].hi_y, fa[i].hi_x - fa[i].lo_x + 1, fa[i].hi_y - fa[i].lo_y + 1,
               fb[j].sep_x, fb[j].sep_y, fb[j].cluster, fb[j].lo_x, fb[j].lo_y, fb[j].hi_x, fb[j].hi_y, m, n, fb[j].sep_x, fb[j].sep_y, level, interval);
      if (n != fa[i].hi_x - fa[i].lo_x + 1) { chol_set_error("TRSM: B tile width %d != pivot size %d", n, fa[i].hi_x - fa[i].lo_x + 1); return CHOLAMD_ERR_ARG; }
      chol_trsm_desc t = { 0, 0, poff(tile_ptr(rB, &fb[j])), n, rA->ld, m, rB->ld };
      rows.push_back(t);
    }
    if ((rc = run_trsm(Lp, n, rA->ld, rows, (hipStream_t)stream))) return rc;
  }
  return 0;
}

static int fused_update(const cholamd_region *rA, const cholamd_region *rB, const cholamd_region *rC,
                        const cholamd_filled *fa, int nA, const cholamd_filled *fb, int nB, const cholamd_filled *fc, int nC,
                        int ccs, int level, int interval, int debug, void *stream, bool is_syrk)
{
  int rc = have_device();
  if (!rc) rc = region_ok(rA, "rA");
  if (!rc) rc = region_ok(rB, "rB");
  if (!rc) rc = region_ok(rC, "rC");
  if (rc) return rc;
  std::vector<chol_upd_task> tasks;
  std::vector<chol_upd_src> srcs;
  for (int i = 0; i < nA; i++) {
    const cholamd_filled &a = fa[i];
    if ((rc = tile_inside(rA, &a))) return rc;
    const int row = a.cluster, sAx = a.hi_x - a.lo_x + 1, sAy = a.hi_y - a.lo_y + 1;
    for (int j = 0; j < nB; j++) {
      const cholamd_filled &b = fb[j];
      if ((rc = tile_inside(rB, &b))) return rc;
      const int col = b.cluster, sBx = b.hi_x - b.lo_x + 1;
      const int cz = row * ccs + col;
      const cholamd_filled *c = nullptr;
      for (int k = 0; k < nC; k++) // the reference's linear search, blas.rg:385-392 / 468-475
        if (fc[k].sep_x == a.sep_x && fc[k].sep_y == b.sep_x && fc[k].cluster == cz) { c = &fc[k]; break; }
      if (!c) continue;
      if ((rc = tile_inside(rC, c))) return rc;
      const int sCx = c->hi_x - c->lo_x + 1, sCy = c->hi_y - c->lo_y + 1;
      if (sCx <= 0 || sCy <= 0) continue;
      if (is_syrk && col > row) continue;
      if (debug)
        printf("GEMM: {'A': (%d, %d, %d), 'A_Lo': (%d, %d), 'A_Hi': (%d, %d), 'sizeA': (%d, %d), 'B': (%d, %d, %d), 'B_Lo': (%d, %d), 'B_Hi': (%d, %d), 'sizeB': (%d, %d), 'C': (%d, %d, %d), 'C_Lo': (%d, %d), 'C_Hi': (%d, %d), 'sizeC': (%d, %d), 'Block': (%d, %d), 'Level': %d, 'Interval': %d}\n",
               a.sep_x, a.sep_y, a.cluster, a.lo_x, a.lo_y, a.hi_x, a.hi_y, sAx, sAy, b.sep_x, b.sep_y, b.cluster, b.lo_x, b.lo_y, b.hi_x, b.hi_y, sBx, b.hi_y - b.lo_y + 1,
               c->sep_x, c->sep_y, c->cluster, c->lo_x, c->lo_y, c->hi_x, c->hi_y, sCx, sCy, c->sep_x, c->sep_y, level, interval);
      const bool syrk = is_syrk && col == row;
      chol_upd_src s = { poff(tile_ptr(rA, &a)), poff(tile_ptr(rB, &b)), rA->ld, rB->ld, sAy, 0, 0, 0 };
      srcs.push_back(s);
      // distinct (a, b) pairs address distinct C tiles inside one fused task, so one source per task group
      add_update_tasks(tasks, (int)srcs.size() - 1, (int)srcs.size(), tile_ptr(rC, c), rC->ld, syrk ? sCx : sAx, syrk ? sCx : sBx, syrk);
    }
  }
  return run_updates(tasks, srcs, (hipStream_t)stream);
}

extern "C" int cholamd_fused_dsyrk(const cholamd_region *rA, const cholamd_region *rB, const cholamd_region *rC,
                                   const cholamd_filled *fa, int nA, const cholamd_filled *fb, int nB, const cholamd_filled *fc, int nC,
                                   int ccs, int level, int interval, int debug, void *stream)
{
  return fused_update(rA, rB, rC, fa, nA, fb, nB, fc, nC, ccs, level, interval, debug, stream, true);
}
extern "C" int cholamd_fused_dgemm(const cholamd_region *rA, const cholamd_region *rB, const cholamd_region *rC,
                                   const cholamd_filled *fa, int nA, const cholamd_filled *fb, int nB, const cholamd_filled *fc, int nC,
                                   int ccs, int level, int interval, int debug, void *stream)
{
  return fused_update(rA, rB, rC, fa, nA, fb, nB, fc, nC, ccs, level, interval, debug, stream, false);
}

// ---- the reference's debug mode: the main loop of mmat.rg:1227-1355 literally, one fused task at a time, with write_blocks dumps
static int debug_dump(cholamd_device *d, const double *d_arena, std::vector<double> &host, const char *dir, int level, const char *op,
                      int ax, int ay, int bx, int by, int cx, int cy, int full)
{
  const cholamd_plan *p = d->plan;
  HIPCHK(hipMemcpy(host.data(), d_arena, (size_t)p->arena * sizeof(double), hipMemcpyDeviceToHost));
  char stem[1100], file[1200], header[200];
  if (!std::strcmp(op, "POTRF")) { snprintf(stem, sizeof stem, "%s/potrf_lvl%d_a%d%d", dir, level, ax, ay); snprintf(header, sizeof header, "Level: %d POTRF A=(%d, %d)", level, ax, ay); }
  else if (!std::strcmp(op, "TRSM")) { snprintf(stem, sizeof stem, "%s/trsm_lvl%d_a%d%d_b%d%d", dir, level, ax, ay, bx, by); snprintf(header, sizeof header, "Level: %d TRSM A=(%d, %d) B=(%d, %d)", level, ax, ay, bx, by); }
  else { snprintf(stem, sizeof stem, "%s/gemm_lvl%d_a%d%d_b%d%d_c%d%d", dir, level, ax, ay, bx, by, cx, cy); snprintf(header, sizeof header, "Level: %d GEMM A=(%d, %d) B=(%d, %d) C=(%d, %d)", level, ax, ay, bx, by, cx, cy); }
  snprintf(file, sizeof file, "%s.mtx", stem);
  printf("filename: %s\n", file);
  printf("saving matrix to: %s\n\n", file);
  int rc = cholamd_plan_write_matrix(p, host.data(), file, full);
  if (rc) return rc;
  snprintf(file, sizeof file, "%s.txt", stem);
  printf("filename: %s\n", file);
  return cholamd_plan_write_blocks_txt(p, host.data(), file, header);
}
extern "C" int cholamd_factor_debug(cholamd_device *d, double *d_arena, const char *dir, int full_precision, void *stream)
{
  HIPCHK(hipSetDevice(d->dev));
  const cholamd_plan *p = d->plan;
  const int L = p->levels, ns = p->nsep;
  std::vector<double> host((size_t)p->arena);
  auto region_of = [&](int r, int c) {
    const chol_block *B = chol_plan_block(p, r, c);
    cholamd_region rg = { d_arena + B->off, B->ld, B->lo_x, B->lo_y, B->hi_x, B->hi_y, B->tmap };
    return rg;
  };
  for (int lvl = L - 1; lvl >= 0; lvl--) {
    const int lbl = L - 1 - lvl;
    // filled tiles of the level's snapshot, grouped by block (the snapshot is ordered by (row label, col label, cluster))
    std::vector<std::vector<cholamd_filled>> fl((size_t)(ns + 1) * (ns + 1));
    for (int64_t i = 0; i < p->snap_n[lbl]; i++) fl[(size_t)p->snap[lbl][i].sep_x * (ns + 1) + p->snap[lbl][i].sep_y].push_back(p->snap[lbl][i]);
    auto F = [&](int r, int c) -> std::vector<cholamd_filled> & { return fl[(size_t)r * (ns + 1) + c]; };
    const int h0 = 1 << lvl, h1 = (1 << (lvl + 1)) - 1;
    for (int h = h0; h <= h1; h++) { // POTRF sweep, mmat.rg:1240-1257
      const int s = p->tree[h];
      cholamd_region rA = region_of(s, s);
      int rc = cholamd_fused_dpotrf(&rA, F(s, s).data(), (int)F(s, s).size(), lvl, lbl, 1, stream);
      if (rc < 0) return rc;
      if (rc > 0) { int h2[2] = { rc, s }; HIPCHK(hipMemcpy(d->info, h2, sizeof h2, hipMemcpyHostToDevice)); d->info_last = d->info; d->info_foreign = true; }
      if ((rc = debug_dump(d, d_arena, host, dir, lvl, "POTRF", s, s, 0, 0, 0, 0, full_precision))) return rc;
    }
    for (int h = h0; h <= h1; h++) { // TRSM sweep, mmat.rg:1259-1291
      const int s = p->tree[h];
      for (int hp = h / 2; hp >= 1; hp /= 2) {
        const int par = p->tree[hp];
        cholamd_region rA = region_of(s, s), rB = region_of(par, s);
        int rc = cholamd_fused_dtrsm(&rA, &rB, F(s, s).data(), (int)F(s, s).size(), F(par, s).data(), (int)F(par, s).size(), lvl, lbl, 1, stream);
        if (rc) return rc;
        if ((rc = debug_dump(d, d_arena, host, dir, lvl, "TRSM", s, s, par, s, 0, 0, full_precision))) return rc;
      }
    }
    for (int h = h0; h <= h1; h++) { // SYRK / GEMM sweep, mmat.rg:1293-1347
      const int s = p->tree[h];
      for (int hp = h / 2; hp >= 1; hp /= 2) {
        const int par = p->tree[hp];
        const int ccs = cholamd_plan_ntiles_at_level(p, par, lvl);
        for (int hg = hp; hg >= 1; hg /= 2) {
          const int gp = p->tree[hg];
          cholamd_region rA = region_of(gp, s), rB = region_of(par, s), rC = region_of(gp, par);
          int rc = (gp == par ? cholamd_fused_dsyrk : cholamd_fused_dgemm)(&rA, &rB, &rC, F(gp, s).data(), (int)F(gp, s).size(), F(par, s).data(), (int)F(par, s).size(),
                                                                             F(gp, par).data(), (int)F(gp, par).size(), ccs, lvl, lbl, 1, stream);
          if (rc) return rc;
          if ((rc = debug_dump(d, d_arena, host, dir, lvl, "GEMM", gp, s, par, s, gp, par, full_precision))) return rc;
        }
      }
    }
  }
  return 0;
}

// ---- L-A: device-pointer BLAS ----------------------------------------------------------------
extern "C" int cholamd_dpotrf_dev(int n, double *d_a, int lda, int *d_info, void *stream)
{
  int rc = have_device();
  if (rc) return rc;
  if (n < 0 || lda < (n > 1 ? n : 1)) { chol_set_error("dpotrf: bad n/lda"); return CHOLAMD_ERR_ARG; }
  if (n == 0) return 0;
  if ((rc = check_ptr(d_a, "a"))) return rc;
  std::vector<chol_potrf_desc> v(1);
  v[0] = { poff(d_a), 0, n, lda, 0, 0 };
  int info = 0;
  rc = run_potrf(v, (hipStream_t)stream, &info, nullptr);
  if (rc) return rc;
  if (d_info) HIPCHK(hipMemcpy(d_info, &info, sizeof(int), hipMemcpyHostToDevice));
  return info;
}
extern "C" int cholamd_dtrsm_dev(int m, int n, const double *d_a, int lda, double *d_b, int ldb, void *stream)
{
  int rc = have_device();
  if (rc) return rc;
  if (m < 0 || n < 0 || lda < (n > 1 ? n : 1) || ldb < (m > 1 ? m : 1)) { chol_set_error("dtrsm: bad sizes"); return CHOLAMD_ERR_ARG; }
  if (m == 0 || n == 0) return 0;
  if ((rc = check_ptr(d_a, "a")) || (rc = check_ptr(d_b, "b"))) return rc;
  std::vector<chol_trsm_desc> rows(1);
  rows[0] = { 0, 0, poff(d_b), n, lda, m, ldb };
  return run_trsm(d_a, n, lda, rows, (hipStream_t)stream);
}
extern "C" int cholamd_dgemm_dev(int m, int n, int k, const double *d_a, int lda, const double *d_b, int ldb, double *d_c, int ldc, void *stream)
{
  int rc = have_device();
  if (rc) return rc;
  if (m < 0 || n < 0 || k < 0 || lda < (m > 1 ? m : 1) || ldb < (n > 1 ? n : 1) || ldc < (m > 1 ? m : 1)) { chol_set_error("dgemm: bad sizes"); return CHOLAMD_ERR_ARG; }
  if (m == 0 || n == 0 || k == 0) return 0;
  if ((rc = check_ptr(d_a, "a")) || (rc = check_ptr(d_b, "b")) || (rc = check_ptr(d_c, "c"))) return rc;
  std::vector<chol_upd_task> tasks;
  std::vector<chol_upd_src> srcs(1);
  srcs[0] = { poff(d_a), poff(d_b), lda, ldb, k, 0 };
  add_update_tasks(tasks, 0, 1, d_c, ldc, m, n, false);
  return run_updates(tasks, srcs, (hipStream_t)stream);
}
extern "C" int cholamd_dsyrk_dev(int n, int k, const double *d_a, int lda, double *d_c, int ldc, void *stream)
{
  int rc = have_device();
  if (rc) return rc;
  if (n < 0 || k < 0 || lda < (n > 1 ? n : 1) || ldc < (n > 1 ? n : 1)) { chol_set_error("dsyrk: bad sizes"); return CHOLAMD_ERR_ARG; }
  if (n == 0 || k == 0) return 0;
  if ((rc = check_ptr(d_a, "a")) || (rc = check_ptr(d_c, "c"))) return rc;
  std::vector<chol_upd_task> tasks;
  std::vector<chol_upd_src> srcs(1);
  srcs[0] = { poff(d_a), poff(d_a), lda, lda, k, 0 };
  add_update_tasks(tasks, 0, 1, d_c, ldc, n, n, true);
  return run_updates(tasks, srcs, (hipStream_t)stream);
}
extern "C" int cholamd_dtrsv_dev(int trans, int n, const double *d_a, int lda, double *d_x, void *stream)
{
  int rc = have_device();
  if (rc) return rc;
  if (n < 0 || lda < (n > 1 ? n : 1) || (trans != CholamdNoTrans && trans != CholamdTrans)) { chol_set_error("dtrsv: bad arguments"); return CHOLAMD_ERR_ARG; }
  if (n == 0) return 0;
  if ((rc = check_ptr(d_a, "a")) || (rc = check_ptr(d_x, "x"))) return rc;
  hipStream_t st = (hipStream_t)stream;
  scratch sc;
  chol_trsv_desc t = { poff(d_a), n, lda, 0, 0 };
  chol_trsv_desc *dt;
  if ((rc = sc.put(&dt, &t, 1, st))) return rc;
  if (trans == CholamdNoTrans) {
    HIPCHK((hipError_t)chol_launch_trsv_fwd(nullptr, dt, 1, d_x, st));
  } else {
    int zero2[2] = { 0, 0 };
    int *ds;
    if ((rc = sc.put(&ds, zero2, 2, st))) return rc;
    HIPCHK((hipError_t)chol_launch_bwd(nullptr, dt, nullptr, ds, 1, d_x, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
extern "C" int cholamd_dgemv_dev(int trans, int m, int n, const double *d_a, int lda, const double *d_x, double *d_y, void *stream)
{
  int rc = have_device();
  if (rc) return rc;
  if (m < 0 || n < 0 || lda < (m > 1 ? m : 1) || (trans != CholamdNoTrans && trans != CholamdTrans)) { chol_set_error("dgemv: bad arguments"); return CHOLAMD_ERR_ARG; }
  if (m == 0 || n == 0) return 0;
  if ((rc = check_ptr(d_a, "a")) || (rc = check_ptr(d_x, "x")) || (rc = check_ptr(d_y, "y"))) return rc;
  hipStream_t st = (hipStream_t)stream;
  scratch sc;
  if (trans == CholamdNoTrans) { // y(m) -= A x(n): the forward kernel with pointer-valued offsets
    std::vector<chol_gemv_desc> g;
    std::vector<int> gs, gr;
    for (int row0 = 0; row0 < m; row0 += 256) {
      gs.push_back((int)g.size());
      gr.push_back(row0); gr.push_back(0);
      chol_gemv_desc d = { poff(d_a), m, n, lda, 0, 0 };
      g.push_back(d);
    }
    gs.push_back((int)g.size());
    // vectors are addressed relative to y: x_off = x - y in doubles
    for (auto &d : g) d.x_off = (int)(poff(d_x) - poff(d_y));
    chol_gemv_desc *dg; int *dgs, *dgr;
    if ((rc = sc.put(&dg, g.data(), g.size(), st)) || (rc = sc.put(&dgs, gs.data(), gs.size(), st)) || (rc = sc.put(&dgr, gr.data(), gr.size(), st))) return rc;
    if (poff(d_x) - poff(d_y) != (int64_t)(int)(poff(d_x) - poff(d_y))) { chol_set_error("dgemv: x and y too far apart"); return CHOLAMD_ERR_ARG; }
    HIPCHK((hipError_t)chol_launch_gemv_fwd(nullptr, dg, dgs, dgr, (int)gs.size() - 1, d_y, st));
  } else { // y(n) -= A^T x(m): the backward kernel with an empty triangle (n = 0) does only the gather
    chol_trsv_desc t = { 0, 0, 1, 0, 0 };
    chol_gemv_desc d = { poff(d_a), m, n, lda, (int)(poff(d_x) - poff(d_y)), 0 };
    if (poff(d_x) - poff(d_y) != (int64_t)d.x_off) { chol_set_error("dgemv: x and y too far apart"); return CHOLAMD_ERR_ARG; }
    int start[2] = { 0, 1 };
    chol_trsv_desc *dt; chol_gemv_desc *dg; int *ds;
    if ((rc = sc.put(&dt, &t, 1, st)) || (rc = sc.put(&dg, &d, 1, st)) || (rc = sc.put(&ds, start, 2, st))) return rc;
    HIPCHK((hipError_t)chol_launch_bwd(nullptr, dt, dg, ds, 1, d_y, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// ---- L-A: host-pointer CBLAS / LAPACKE replacements -------------------------------------------
static thread_local int g_blas_status = 0;
extern "C" int cholamd_blas_status(void) { return g_blas_status; }
extern "C" void cholamd_openblas_set_num_threads(int) {} // mmat.rg:1057: parallelism is the GPU's

struct host_mat { // a host matrix mirrored on the device for the duration of one call
  dev_buf<double> d; double *h = nullptr; int rows = 0, cols = 0, ld = 0; bool writeback = false;
  int up(const double *hp, int r, int c, int ldh, bool wb)
  {
    h = const_cast<double *>(hp); rows = r; cols = c; ld = ldh; writeback = wb;
    if (r == 0 || c == 0) return 0;
    { int rc = d.alloc((size_t)ld * cols); if (rc) return rc; }
    HIPCHK(hipMemcpy(d, h, ((size_t)ld * (cols - 1) + rows) * sizeof(double), hipMemcpyHostToDevice));
    return 0;
  }
  int down()
  {
    if (d && writeback) HIPCHK(hipMemcpy2D(h, (size_t)ld * sizeof(double), d, (size_t)ld * sizeof(double), (size_t)rows * sizeof(double), cols, hipMemcpyDeviceToHost));
    return 0;
  }
};

extern "C" int cholamd_LAPACKE_dpotrf(int layout, char uplo, int n, double *a, int lda)
{
  g_blas_status = 0;
  if (layout != CholamdColMajor || (uplo != 'L' && uplo != 'l')) { chol_set_error("LAPACKE_dpotrf: only ColMajor/'L' (blas.rg:71)"); return g_blas_status = CHOLAMD_ERR_ARG; }
  int rc = have_device();
  if (rc) return g_blas_status = rc;
  if (n == 0) return 0;
  host_mat A;
  if ((rc = A.up(a, n, n, lda, true))) return g_blas_status = rc;
  int info = cholamd_dpotrf_dev(n, A.d, lda, nullptr, nullptr);
  if (info < 0) return g_blas_status = info;
  if ((rc = A.down())) return g_blas_status = rc;
  return info;
}
extern "C" void cholamd_cblas_dtrsm(int layout, int side, int uplo, int transa, int diag, int m, int n, double alpha,
                                    const double *a, int lda, double *b, int ldb)
{
  g_blas_status = 0;
  if (layout != CholamdColMajor || side != CholamdRight || uplo != CholamdLower || transa != CholamdTrans || diag != CholamdNonUnit || alpha != 1.0) {
    chol_set_error("cblas_dtrsm: only ColMajor/Right/Lower/Trans/NonUnit/alpha=1 (blas.rg:99)");
    g_blas_status = CHOLAMD_ERR_ARG; return;
  }
  int rc = have_device();
  if (rc) { g_blas_status = rc; return; }
  host_mat A, B;
  if ((rc = A.up(a, n, n, lda, false)) || (rc = B.up(b, m, n, ldb, true))) { g_blas_status = rc; return; }
  if ((rc = cholamd_dtrsm_dev(m, n, A.d, lda, B.d, ldb, nullptr)) || (rc = B.down())) g_blas_status = rc;
}
extern "C" void cholamd_cblas_dgemm(int layout, int transa, int transb, int m, int n, int k, double alpha, const double *a, int lda,
                                    const double *b, int ldb, double beta, double *c, int ldc)
{
  g_blas_status = 0;
  if (layout != CholamdColMajor || transa != CholamdNoTrans || transb != CholamdTrans || alpha != -1.0 || beta != 1.0) {
    chol_set_error("cblas_dgemm: only ColMajor/NoTrans/Trans/alpha=-1/beta=1 (blas.rg:139)");
    g_blas_status = CHOLAMD_ERR_ARG; return;
  }
  int rc = have_device();
  if (rc) { g_blas_status = rc; return; }
  host_mat A, B, C;
  if ((rc = A.up(a, m, k, lda, false)) || (rc = B.up(b, n, k, ldb, false)) || (rc = C.up(c, m, n, ldc, true))) { g_blas_status = rc; return; }
  if ((rc = cholamd_dgemm_dev(m, n, k, A.d, lda, B.d, ldb, C.d, ldc, nullptr)) || (rc = C.down())) g_blas_status = rc;
}
extern "C" void cholamd_cblas_dsyrk(int layout, int uplo, int trans, int n, int k, double alpha, const double *a, int lda,
                                    double beta, double *c, int ldc)
{
  g_blas_status = 0;
  if (layout != CholamdColMajor || uplo != CholamdLower || trans != CholamdNoTrans || alpha != -1.0 || beta != 1.0) {
    chol_set_error("cblas_dsyrk: only ColMajor/Lower/NoTrans/alpha=-1/beta=1 (blas.rg:187)");
    g_blas_status = CHOLAMD_ERR_ARG; return;
  }
  int rc = have_device();
  if (rc) { g_blas_status = rc; return; }
  host_mat A, C;
  if ((rc = A.up(a, n, k, lda, false)) || (rc = C.up(c, n, n, ldc, true))) { g_blas_status = rc; return; }
  if ((rc = cholamd_dsyrk_dev(n, k, A.d, lda, C.d, ldc, nullptr)) || (rc = C.down())) g_blas_status = rc;
}
extern "C" void cholamd_cblas_dtrsv(int layout, int uplo, int transa, int diag, int n, const double *a, int lda, double *x, int incx)
{
  g_blas_status = 0;
  if (layout != CholamdColMajor || uplo != CholamdLower || diag != CholamdNonUnit || incx != 1 || (transa != CholamdNoTrans && transa != CholamdTrans)) {
    chol_set_error("cblas_dtrsv: only ColMajor/Lower/NonUnit/incx=1 (blas.rg:226)");
    g_blas_status = CHOLAMD_ERR_ARG; return;
  }
  int rc = have_device();
  if (rc) { g_blas_status = rc; return; }
  host_mat A, X;
  if ((rc = A.up(a, n, n, lda, false)) || (rc = X.up(x, n, 1, n > 1 ? n : 1, true))) { g_blas_status = rc; return; }
  if ((rc = cholamd_dtrsv_dev(transa, n, A.d, lda, X.d, nullptr)) || (rc = X.down())) g_blas_status = rc;
}
extern "C" void cholamd_cblas_dgemv(int layout, int trans, int m, int n, double alpha, const double *a, int lda, const double *x, int incx,
                                    double beta, double *y, int incy)
{
  g_blas_status = 0;
  if (layout != CholamdColMajor || alpha != -1.0 || beta != 1.0 || incx != 1 || incy != 1 || (trans != CholamdNoTrans && trans != CholamdTrans)) {
    chol_set_error("cblas_dgemv: only ColMajor/alpha=-1/beta=1/inc=1 (blas.rg:263)");
    g_blas_status = CHOLAMD_ERR_ARG; return;
  }
  int rc = have_device();
  if (rc) { g_blas_status = rc; return; }
  const int lx = trans == CholamdNoTrans ? n : m, ly = trans == CholamdNoTrans ? m : n;
  if (m == 0 || n == 0) return;
  // x and y share one device buffer so that 32-bit relative offsets always suffice
  dev_buf<double> xy;
  if (xy.alloc((size_t)(lx + ly))) { g_blas_status = CHOLAMD_ERR_HIP; return; }
  host_mat A;
  rc = A.up(a, m, n, lda, false);
  if (!rc && hipMemcpy(xy, x, (size_t)lx * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = CHOLAMD_ERR_HIP;
  if (!rc && hipMemcpy(xy + lx, y, (size_t)ly * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = CHOLAMD_ERR_HIP;
  if (!rc) rc = cholamd_dgemv_dev(trans, m, n, A.d, lda, xy, xy + lx, nullptr);
  if (!rc && hipMemcpy(y, xy + lx, (size_t)ly * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = CHOLAMD_ERR_HIP;
  g_blas_status = rc;
}
