// C ABI glue of libcholamd: device objects, the level schedule, the task-level (fused_*) and the
// BLAS-level entry points.  Compiled with hipcc; everything exported is extern "C" (include/cholamd.h).
// There is no CPU fallback: every compute entry point needs a HIP device and fails loudly otherwise.
#include "chol_device.h"

int no_device_error()
{
  chol_set_error("no usable HIP device (libcholamd has no CPU fallback)");
  return CHOLAMD_ERR_NO_DEVICE;
}
// do [a, a + na) and [b, b + nb) share a byte?  (the argument checks of the gradients, the products and the Schur entry points)
bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
  const char *pa = (const char *)a, *pb = (const char *)b;
  return pa < pb + nb && pb < pa + na;
}

extern "C" int cholamd_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// Every allocation of floating-point data goes through fp_malloc.  With CHOLAMD_POISON set and non-zero (read at each allocation) it takes a
// guard tail of CHOL_POISON_GUARD bytes more and fills the whole allocation with 0xFF bytes -- a NaN in fp64 and fp32 -- before any clearing the
// caller does: a kernel that reads a value it does not own, even to multiply it by zero, then produces NaN.  Integer, flag and descriptor
// buffers are never poisoned (bounded spin-waits read some of them).  Unset: a plain hipMalloc.
#define CHOL_POISON_GUARD ((size_t)64 << 10)
static bool poison_on()
{
  const char *e = std::getenv("CHOLAMD_POISON");
  return e && *e && atoi(e) != 0;
}
static hipError_t poison_fill(void *p, size_t bytes)
{
  hipError_t e = hipMemset(p, 0xFF, bytes);
  return e == hipSuccess ? hipDeviceSynchronize() : e; // ordered before work on any stream
}
static hipError_t fp_malloc(void **dptr, size_t bytes)
{
  if (!poison_on()) return hipMalloc(dptr, bytes);
  hipError_t e = hipMalloc(dptr, bytes + CHOL_POISON_GUARD);
  if (e == hipSuccess && (e = poison_fill(*dptr, bytes + CHOL_POISON_GUARD)) != hipSuccess) { (void)hipFree(*dptr); *dptr = nullptr; }
  return e;
}

// What chol_devbuf.h's owners are made of: every device buffer of the library's own comes from and goes back through these.  The release is a
// synchronous hipFree: re-allocations rely on it waiting for the work in flight.
static std::atomic<int64_t> g_live_buffers{ 0 };
int chol_dev_acquire(void **p, size_t bytes, int floating_point)
{
  void *q = *p = nullptr;
  HIPCHK(floating_point ? fp_malloc(&q, bytes) : hipMalloc(&q, bytes));
  if ((*p = q)) g_live_buffers++; // (an allocation of zero bytes is no buffer)
  return 0;
}
void chol_dev_release(void *p) { (void)hipFree(p); g_live_buffers--; }
// The clearing runs on the null stream, and a caller's stream may be non-blocking (torch's pool streams are): it does not wait for the null stream, and
// the buffer is used by kernels on the caller's stream in the same call.  So the device is synchronised, like the poison fill: ordered before work on any
// stream.  Creation and first use only (the "repeated calls allocate nothing" tests keep it off the hot path).
int chol_dev_zero(void *p, size_t bytes)
{
  HIPCHK(hipMemset(p, 0, bytes));
  HIPCHK(hipDeviceSynchronize());
  return 0;
}
int chol_dev_copy_in(void *p, const void *host, size_t bytes) { HIPCHK(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice)); return 0; }
extern "C" int64_t cholamd_debug_live_buffers(void) { return g_live_buffers.load(); }

static void free_solve_lists(cholamd_device *d)
{
  d->sv.clear(); d->solve_ready = false;
  d->w256.reset(); d->dg_desc.reset(); d->dg_prefix.reset(); d->zr_sub.reset(); d->n_dg = 0; d->n_zr_sub = 0;
}
static int upload_level(level_dev &l, const chol_level_work &w, bool with_tables = true)
{
  l.n_potrf = w.n_potrf; l.n_trsm = w.n_trsm; l.n_task = w.n_task; l.n_src = w.n_src;
  l.phase.assign(w.phase, w.phase + w.n_phase);
  l.bcast.assign(w.bcast, w.bcast + w.n_bcast);
  // the POTRF descriptors travel with their role tables (chol_potrf_table) behind them in one buffer: desc.tab = byte offset from the descriptor itself
  int rc = 0;
  if (w.n_potrf > 0 && with_tables && !std::getenv("CHOLAMD_NO_ROLE_TABLES")) { // the switch: A/B and the parity test against the in-kernel construction
    const size_t dbytes = ((size_t)w.n_potrf * sizeof(chol_potrf_desc) + 15) / 16 * 16;
    std::vector<unsigned char> buf(dbytes + (size_t)w.n_potrf * CHOL_RR_TAB_BYTES);
    for (int i = 0; i < w.n_potrf; i++) {
      chol_potrf_desc pd = w.potrf[i];
      if (pd.n <= CHOL_RR_MAXN) {
        const size_t at = dbytes + (size_t)i * CHOL_RR_TAB_BYTES;
        pd.tab = (int)(at - (size_t)i * sizeof(chol_potrf_desc)); // relative to the descriptor itself: launches take sub-ranges of the array
        chol_potrf_table(pd.n, pd.sky, buf.data() + at);
      }
      std::memcpy(buf.data() + (size_t)i * sizeof(chol_potrf_desc), &pd, sizeof pd);
    }
    rc = l.potrf.upload_bytes(buf.data(), buf.size());
  } else rc = l.potrf.upload(w.potrf, (size_t)w.n_potrf);
  if (!rc) rc = l.trsm.upload(w.trsm, (size_t)w.n_trsm);
  if (!rc) rc = l.task.upload(w.task, (size_t)w.n_task);
  if (!rc) rc = l.task_mt.upload(w.task_mt, (size_t)w.n_task_mt);
  if (!rc) rc = l.src.upload(w.src, (size_t)w.n_src);
  return rc;
}

static int build_levels(cholamd_device *d)
{
  d->lv.clear(); d->lv32.clear(); d->prog = level_dev(); d->prog_ready = false; // the schedule before this one
  d->jobs.reset(); d->pwaits.reset(); d->exts.reset(); d->pctr.reset(); d->pctr_total.reset();
  d->sched_gen++;
  const int L = d->plan->levels;
  d->lv.resize(L);
  for (int lvl = 0; lvl < L; lvl++) {
    chol_level_work w;
    int rc = chol_build_level_work(d->plan, &d->opt, lvl, d->rank, d->world, &w);
    if (rc) return rc;
    rc = upload_level(d->lv[lvl], w);
    chol_level_work_free(&w);
    if (rc) return rc;
  }
  // single GPU, small problem: the same factorisation as one program launch (the per-level lists above stay for level
  // ranges, the partitioned run and the per-launch timing)
  if (d->world == 1 && d->opt.program) {
    chol_level_work w;
    chol_program g;
    // Liveness is a property of the job list: a follower is queued ahead of some strips it follows, so progress needs a minimum of
    // co-resident workgroups.  The list is simulated here, for every plan and option set, with FOUR resident workgroups and counters
    // raised only on job completion (stricter than the device): a program that cannot make progress that way is not used -- the
    // level-by-level lists below are.  (A GPU shared with other kernels or streams only delays jobs: every wait is bounded by ~2 s.)
    const bool built = chol_build_program(d->plan, &d->opt, &w, &g) == 0;
    const bool live = built && chol_program_check_built(d->plan, &d->opt, 4, &w, &g) == 0;
    if (built && !live) { chol_level_work_free(&w); chol_program_free(&g); }
    if (live) {
      int rc = upload_level(d->prog, w);
      std::vector<int> tot(g.ctr_total, g.ctr_total + g.n_ctr);
      int ncu = 256;
      hipDeviceProp_t prop;
      if (hipGetDeviceProperties(&prop, d->dev) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount;
      d->prog_grid = g.n_job < ncu ? g.n_job : ncu;
      tot.push_back(g.n_job + d->prog_grid); // the queue head: every workgroup draws one index past the end
      int mx = 1;
      for (int t : tot) mx = t > mx ? t : mx;
      d->prog_epoch_limit = (1 << 30) / mx;
      d->n_job = g.n_job; d->n_pctr = (int)tot.size(); d->prog_epoch = 0;
      d->jobs_host.assign(g.job, g.job + g.n_job);
      if (!rc) rc = d->jobs.upload(g.job, (size_t)g.n_job);
      const chol_wait no_wait = { 0, 0 };
      chol_ext no_ext;
      std::memset(&no_ext, 0, sizeof no_ext);
      if (!rc) rc = g.n_wait > 0 ? d->pwaits.upload(g.wait, (size_t)g.n_wait) : d->pwaits.upload(&no_wait, (size_t)1);
      if (!rc) rc = g.n_ext > 0 ? d->exts.upload(g.ext, (size_t)g.n_ext) : d->exts.upload(&no_ext, (size_t)1);
      if (!rc) rc = d->pctr_total.upload(tot.data(), tot.size());
      if (!rc) rc = d->pctr.alloc_zero(tot.size());
      chol_level_work_free(&w);
      chol_program_free(&g);
      if (rc) return rc;
      d->prog_ready = d->n_job > 0;
    }
  }
  return 0;
}

extern "C" int cholamd_device_create(const cholamd_plan *plan, int device_id, cholamd_device **out)
{
  *out = nullptr;
  if (!plan) { chol_set_error("null plan"); return CHOLAMD_ERR_ARG; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return no_device_error();
  if (device_id < 0 || device_id >= ndev) { chol_set_error("device %d out of range (%d devices)", device_id, ndev); return CHOLAMD_ERR_NO_DEVICE; }
  HIPCHK(hipSetDevice(device_id));
  cholamd_device *d = new cholamd_device();
  d->plan = plan; d->dev = device_id;
  chol_sched_opts_from_env(&d->opt);
  { const char *e = getenv("CHOLAMD_SOLVE_REFERENCE_SHAPE"); d->solve_reference_shape = e && *e && atoi(e) != 0; }
  { const char *e = getenv("CHOLAMD_SOLVE_DETERMINISTIC"); d->solve_deterministic = e && *e && atoi(e) != 0; }
  { const char *e = getenv("CHOLAMD_SOLVE_DETERMINISTIC_BLOCK"); d->solve_deterministic_block = e && *e && atoi(e) != 0; }
  { const char *e = getenv("CHOLAMD_SCHUR_DETERMINISTIC"); d->schur_deterministic = e && *e && atoi(e) != 0; }
  { const char *e = getenv("CHOLAMD_MULTIPLY_NRHS_MIN"); d->multiply_nrhs_min = e && *e ? atoi(e) : 0; }
  int rc = build_levels(d);
  if (!rc) rc = d->ws.alloc((size_t)(plan->ws_doubles > 0 ? plan->ws_doubles : 1));
  if (!rc) rc = d->info.alloc_zero(4);
  if (!rc) rc = d->progress.alloc_zero((size_t)(plan->nsep + 2));
  if (!rc) rc = d->a_dst.upload(plan->a_dst, (size_t)plan->nnz_a);
  if (!rc) rc = d->a_val.upload(plan->a_val, (size_t)plan->nnz_a);
  if (!rc) rc = d->perm.upload(plan->perm, (size_t)plan->n);
  if (rc) { cholamd_device_destroy(d); return rc; }
  *out = d;
  return 0;
}

extern "C" void cholamd_device_destroy(cholamd_device *d)
{
  if (!d) return;
  (void)hipSetDevice(d->dev);
  for (auto &a : d->vmm) { // sharded arenas the caller did not free
    (void)hipDeviceSynchronize();
    (void)hipMemUnmap(a.va, a.total);
    for (auto h : a.handles) (void)hipMemRelease(h);
    (void)hipMemAddressFree(a.va, a.total);
  }
  for (auto &t : d->tl) { d->pool.push_back(t.a); d->pool.push_back(t.b); }
  for (auto e : d->pool) (void)hipEventDestroy(e);
  delete d; // with every buffer it owns
}

extern "C" int cholamd_device_set_partition(cholamd_device *d, int rank, int world)
{
  HIPCHK(hipSetDevice(d->dev));
  if (world < 1 || (world & (world - 1)) || rank < 0 || rank >= world || chol_split_level(world) > d->plan->levels - 1) {
    chol_set_error("bad partition: rank %d of %d for a %d-level tree", rank, world, d->plan->levels);
    return CHOLAMD_ERR_ARG;
  }
  d->rank = rank; d->world = world;
  free_solve_lists(d); // rebuilt for the new partition at the next solve
  return build_levels(d);
}

extern "C" int cholamd_device_bcast_phases(const cholamd_device *d)
{ // broadcast phases (CHOL_PH_BCAST: top levels distributed by column blocks, option dist_top) in the device's per-level lists; > 0: the
  // factorisation needs a communicator (cholamd_factor_sharded / cholamd_factor_multi)
  int n = 0;
  for (const level_dev &l : d->lv) for (const chol_phase &ph : l.phase) n += ph.kind == CHOL_PH_BCAST;
  return n;
}
extern "C" int cholamd_device_set_option(cholamd_device *d, const char *name, int value)
{
  HIPCHK(hipSetDevice(d->dev));
  const std::string n(name ? name : "");
  bool rebuild = true;
  if (n == "split_min") d->opt.split_min = value;
  else if (n == "split_nb") d->opt.split_nb = value;
  else if (n == "fuse") d->opt.fuse = value != 0;
  else if (n == "fuse_update_max") d->opt.fuse_update_max = value;
  else if (n == "mt_min_tiles") d->opt.mt_min_tiles = value;
  else if (n == "cells") d->opt.cells = value != 0;
  else if (n == "program") d->opt.program = value != 0;
  else if (n == "follow") d->opt.follow = value != 0;
  else if (n == "super_blocks") d->opt.super_blocks = value;
  else if (n == "follow_tail") d->opt.follow_tail = value;
  else if (n == "follow_tail_split") d->opt.follow_tail_split = value;
  else if (n == "follow_own") d->opt.follow_own = value < 0 ? 0 : value > 2 ? 2 : value;
  else if (n == "staged") d->opt.staged = value != 0;
  else if (n == "fine_upd") d->opt.fine_upd = value != 0;
  else if (n == "skyline") d->opt.skyline = value != 0;
  else if (n == "merge_targets") d->opt.merge_targets = value != 0;
  else if (n == "leaf_envelope") d->opt.leaf_envelope = value != 0;
  else if (n == "trsm_wt_min") d->opt.trsm_wt_min = value < 0 ? 0 : value;
  else if (n == "stage_chunk") d->opt.stage_chunk = value < 0 ? 0 : value;
  else if (n == "dist_top") d->opt.dist_top = value;
  else if (n == "solve_reference_shape") { d->solve_reference_shape = value != 0; rebuild = false; }
  else if (n == "solve_deterministic") { d->solve_deterministic = value != 0; rebuild = false; }
  else if (n == "solve_deterministic_block") { d->solve_deterministic_block = value != 0; rebuild = false; }
  else if (n == "schur_deterministic") { d->schur_deterministic = value != 0; rebuild = false; }
  else if (n == "multiply_nrhs_min") { d->multiply_nrhs_min = value; rebuild = false; }
  else { chol_set_error("unknown option '%s'", n.c_str()); return CHOLAMD_ERR_ARG; }
  return rebuild ? build_levels(d) : 0;
}

extern "C" int cholamd_device_alloc(cholamd_device *d, int64_t doubles, double **dptr)
{
  HIPCHK(hipSetDevice(d->dev));
  HIPCHK(fp_malloc((void **)dptr, (size_t)doubles * sizeof(double)));
  return 0;
}
extern "C" int cholamd_device_free(cholamd_device *d, double *dptr)
{
  HIPCHK(hipSetDevice(d->dev));
  HIPCHK(hipFree(dptr));
  return 0;
}
extern "C" int cholamd_device_upload(cholamd_device *d, double *d_dst, const double *h_src, int64_t doubles, void *stream)
{
  HIPCHK(hipSetDevice(d->dev));
  HIPCHK(hipMemcpyAsync(d_dst, h_src, (size_t)doubles * sizeof(double), hipMemcpyHostToDevice, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}
extern "C" int cholamd_device_download(cholamd_device *d, double *h_dst, const double *d_src, int64_t doubles, void *stream)
{
  HIPCHK(hipSetDevice(d->dev));
  HIPCHK(hipMemcpyAsync(h_dst, d_src, (size_t)doubles * sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}
extern "C" int cholamd_device_sync(cholamd_device *d, void *stream)
{
  HIPCHK(hipSetDevice(d->dev));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

// ---- per-rank arenas (multi-GPU) -----------------------------------------------------------------
// The ranges of the arena a rank works on: the panels of its subtrees (one contiguous label range per tree level below the cut) and the shared
// top (the tail).  Rank 0 -- which gathers the factor and solves -- and a single-GPU device own everything.
static void owned_ranges(const cholamd_device *d, std::vector<std::pair<int64_t, int64_t>> &out)
{
  const cholamd_plan *p = d->plan;
  out.clear();
  if (d->world <= 1 || d->rank == 0) { out.push_back({ 0, p->arena }); return; }
  for (int s = 1; s <= p->nsep; s++) {
    const int o = chol_owner_of(p, s, d->world);
    if (o >= 0 && o != d->rank) continue;
    const int64_t lo = p->panel_off[s], hi = s < p->nsep ? p->panel_off[s + 1] : p->arena;
    if (!out.empty() && out.back().second == lo) out.back().second = hi; else out.push_back({ lo, hi });
  }
}
// zero what the rank owns (the other ranks' panels are never read on this rank; in a sharded arena they alias one scratch chunk).  A plain
// allocation is cleared whole: whole-arena consumers on a rank other than 0 (writers, arena_to_dense, the debug replay) then read zeros
// where the rank stores nothing
static int clear_owned(cholamd_device *d, void *arena, size_t elem, hipStream_t st)
{
  bool sharded = false;
  for (const auto &v : d->vmm) if (v.va == arena) sharded = true;
  if (!sharded) { HIPCHK(hipMemsetAsync(arena, 0, (size_t)d->plan->arena * elem, st)); return 0; }
  std::vector<std::pair<int64_t, int64_t>> r;
  owned_ranges(d, r);
  for (auto &x : r) HIPCHK(hipMemsetAsync((char *)arena + (size_t)x.first * elem, 0, (size_t)(x.second - x.first) * elem, st));
  return 0;
}
#define CHOL_VMM_CHUNK ((size_t)2 << 20)   /* owned ranges are backed in 2 MB steps */
#define CHOL_VMM_SCRATCH ((size_t)64 << 20) /* the chunk every range of another rank's panels aliases */
// An arena for this rank of cholamd_plan_arena_doubles() elements of elem_bytes (8: fp64, 4: the fp32 factor) whose address range is complete --
// every work descriptor keeps its offset -- but of which only the rank's own panels and the shared top are backed by memory of their own
// (hipMemAddressReserve / hipMemCreate / hipMemMap): the ranges of the other ranks' panels all alias ONE 64 MB scratch chunk (this rank never
// reads them; the fill's scatter of A and the macro-tile kernels' edge reads may touch them).  Rank 0 and single-GPU devices get a plain
// allocation.  *backed_bytes: the device memory the arena really takes.
extern "C" int cholamd_device_alloc_arena(cholamd_device *d, int elem_bytes, void **dptr, int64_t *backed_bytes)
{
  HIPCHK(hipSetDevice(d->dev));
  if (elem_bytes != 4 && elem_bytes != 8) { chol_set_error("alloc_arena: element size %d", elem_bytes); return CHOLAMD_ERR_ARG; }
  const size_t full = (size_t)d->plan->arena * (size_t)elem_bytes;
  if (d->world <= 1 || d->rank == 0) {
    HIPCHK(fp_malloc(dptr, full > 0 ? full : 1));
    if (backed_bytes) *backed_bytes = (int64_t)full;
    return 0;
  }
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = d->dev;
  size_t gran = 0;
  HIPCHK(hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended));
  const size_t G = gran > CHOL_VMM_CHUNK ? gran : CHOL_VMM_CHUNK, total = (full + G - 1) / G * G, scratch = (CHOL_VMM_SCRATCH + G - 1) / G * G;
  std::vector<std::pair<int64_t, int64_t>> own;
  owned_ranges(d, own);
  std::vector<std::pair<size_t, size_t>> back; // owned byte ranges, widened to the chunk size, merged
  for (auto &x : own) {
    const size_t lo = (size_t)x.first * elem_bytes / G * G, hi = std::min(total, ((size_t)x.second * elem_bytes + G - 1) / G * G);
    if (!back.empty() && lo <= back.back().second) back.back().second = std::max(back.back().second, hi); else back.push_back({ lo, hi });
  }
  cholamd_device::vmm_arena A; A.va = nullptr; A.total = total;
  HIPCHK(hipMemAddressReserve(&A.va, total, G, nullptr, 0));
  auto fail = [&](hipError_t e, const char *what) {
    (void)hipMemUnmap(A.va, total);
    for (auto h : A.handles) (void)hipMemRelease(h);
    (void)hipMemAddressFree(A.va, total);
    chol_set_error("alloc_arena: %s: %s", what, hipGetErrorString(e));
    return CHOLAMD_ERR_HIP;
  };
  hipMemGenericAllocationHandle_t hs;
  hipError_t e = hipMemCreate(&hs, scratch, &prop, 0);
  if (e != hipSuccess) { (void)hipMemAddressFree(A.va, total); chol_set_error("alloc_arena: hipMemCreate: %s", hipGetErrorString(e)); return CHOLAMD_ERR_HIP; }
  A.handles.push_back(hs);
  size_t backed = scratch, pos = 0, alias_at = 0, alias_len = 0; // (alias_at, alias_len): the longest view of the scratch chunk
  auto alias = [&](size_t lo, size_t hi) { // [lo, hi) onto the scratch chunk, piece by piece
    for (size_t o = lo; o < hi;) {
      const size_t n = std::min(scratch, hi - o);
      hipError_t e2 = hipMemMap((char *)A.va + o, n, 0, hs, 0);
      if (e2 != hipSuccess) return e2;
      if (n > alias_len) { alias_at = o; alias_len = n; }
      o += n;
    }
    return hipSuccess;
  };
  for (auto &b : back) {
    if ((e = alias(pos, b.first)) != hipSuccess) return fail(e, "hipMemMap (scratch)");
    hipMemGenericAllocationHandle_t h;
    if ((e = hipMemCreate(&h, b.second - b.first, &prop, 0)) != hipSuccess) return fail(e, "hipMemCreate");
    A.handles.push_back(h);
    if ((e = hipMemMap((char *)A.va + b.first, b.second - b.first, 0, h, 0)) != hipSuccess) return fail(e, "hipMemMap");
    backed += b.second - b.first;
    pos = b.second;
  }
  if ((e = alias(pos, total)) != hipSuccess) return fail(e, "hipMemMap (scratch)");
  // access for the rank's own device AND for every peer that can reach it: the local communicator's ordered sum, its peer copies and
  // the gather to rank 0 read other ranks' arenas from their owners' devices, and hipDeviceEnablePeerAccess does not cover memory
  // mapped with hipMemMap
  std::vector<hipMemAccessDesc> acc;
  int ndev = 0;
  (void)hipGetDeviceCount(&ndev);
  for (int q = 0; q < ndev; q++) {
    int can = q == d->dev;
    if (!can && hipDeviceCanAccessPeer(&can, q, d->dev) != hipSuccess) can = 0;
    if (!can) continue;
    hipMemAccessDesc a1 = {};
    a1.location.type = hipMemLocationTypeDevice; a1.location.id = q; a1.flags = hipMemAccessFlagsProtReadWrite;
    acc.push_back(a1);
  }
  if ((e = hipMemSetAccess(A.va, total, acc.data(), acc.size())) != hipSuccess) return fail(e, "hipMemSetAccess");
  if (poison_on()) { // as fp_malloc: the owned ranges (their widening to the chunk size is the guard) and the scratch chunk once
    for (auto &b : back)
      if ((e = poison_fill((char *)A.va + b.first, b.second - b.first)) != hipSuccess) return fail(e, "hipMemset (poison)");
    if (alias_len > 0 && (e = poison_fill((char *)A.va + alias_at, alias_len)) != hipSuccess) return fail(e, "hipMemset (poison)");
  }
  d->vmm.push_back(A);
  *dptr = A.va;
  if (backed_bytes) *backed_bytes = (int64_t)backed;
  return 0;
}
extern "C" int cholamd_device_free_arena(cholamd_device *d, void *dptr)
{
  HIPCHK(hipSetDevice(d->dev));
  for (size_t i = 0; i < d->vmm.size(); i++)
    if (d->vmm[i].va == dptr) {
      HIPCHK(hipDeviceSynchronize());
      (void)hipMemUnmap(dptr, d->vmm[i].total);
      for (auto h : d->vmm[i].handles) (void)hipMemRelease(h);
      (void)hipMemAddressFree(dptr, d->vmm[i].total);
      d->vmm.erase(d->vmm.begin() + i);
      return 0;
    }
  HIPCHK(hipFree(dptr));
  return 0;
}

// ---- timing helpers -------------------------------------------------------------------------
hipEvent_t get_event(cholamd_device *d)
{
  if (!d->pool.empty()) { hipEvent_t e = d->pool.back(); d->pool.pop_back(); return e; }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}

extern "C" int cholamd_device_set_timing(cholamd_device *d, int on)
{
  d->timing = on != 0;
  for (auto &t : d->tl) { d->pool.push_back(t.a); d->pool.push_back(t.b); }
  d->tl.clear();
  return 0;
}
// kinds: 0 potrf (+ fused trsm), 1 trsm, 2 update, 3 program launch, 4 extend-add exchange (RCCL), 5 broadcasts of the distributed top levels
#define CHOL_TIMING_KINDS 8
#define CHOL_TK_EXCHANGE 4
#define CHOL_TK_BCAST 5
extern "C" int cholamd_device_get_timing_ex(cholamd_device *d, float ms_by_kind[CHOL_TIMING_KINDS], int launches_by_kind[CHOL_TIMING_KINDS])
{
  HIPCHK(hipSetDevice(d->dev));
  for (int k = 0; k < CHOL_TIMING_KINDS; k++) { ms_by_kind[k] = 0.f; launches_by_kind[k] = 0; }
  for (auto &t : d->tl) {
    HIPCHK(hipEventSynchronize(t.b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, t.a, t.b));
    ms_by_kind[t.kind] += ms; launches_by_kind[t.kind]++;
    d->pool.push_back(t.a); d->pool.push_back(t.b);
  }
  d->tl.clear();
  return 0;
}
extern "C" int cholamd_device_get_timing(cholamd_device *d, float ms_by_kind[4], int launches_by_kind[4])
{ // the four compute kinds (the exchange kinds of a sharded run: cholamd_device_get_timing_ex)
  float ms[CHOL_TIMING_KINDS]; int n[CHOL_TIMING_KINDS];
  const int rc = cholamd_device_get_timing_ex(d, ms, n);
  if (rc) return rc;
  for (int k = 0; k < 4; k++) { ms_by_kind[k] = ms[k]; launches_by_kind[k] = n[k]; }
  return 0;
}

extern "C" int cholamd_device_event_overhead(cholamd_device *d, void *stream, float *ms_out)
{ // what a (record, record) pair with NOTHING between reads on this stream: the share of every timed launch above that is
  // the event commands themselves, not the kernel (bench.py subtracts it)
  HIPCHK(hipSetDevice(d->dev));
  hipStream_t st = (hipStream_t)stream;
  const int reps = 64;
  std::vector<hipEvent_t> ev(2 * reps);
  for (auto &e : ev) e = get_event(d);
  for (int i = 0; i < reps; i++) { HIPCHK(hipEventRecord(ev[2 * i], st)); HIPCHK(hipEventRecord(ev[2 * i + 1], st)); }
  HIPCHK(hipStreamSynchronize(st));
  double acc = 0.0;
  for (int i = 0; i < reps; i++) { float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1])); acc += ms; }
  for (auto e : ev) d->pool.push_back(e);
  *ms_out = (float)(acc / reps);
  return 0;
}

// ---- the hot path (the program launch; the fill and the level-by-level driver of both precisions: at factor_levels_comm below) ----
extern "C" int cholamd_factor(cholamd_device *d, double *d_arena, void *stream)
{
  if (!d->prog_ready) return cholamd_factor_levels(d, d_arena, d->plan->levels - 1, 0, stream);
  HIPCHK(hipSetDevice(d->dev));
  hipStream_t st = (hipStream_t)stream;
  if (d->info_foreign) { HIPCHK(hipMemsetAsync(d->info, 0, 4 * sizeof(int), st)); d->info_foreign = false; } // another path wrote slot 0 since
  int *const info_cur = d->info + 2 * d->info_parity, *const info_next = d->info + 2 * (d->info_parity ^ 1);
  d->info_parity ^= 1; d->info_last = info_cur;
  // counters are monotonic across factorisations (no reset between them); they start over, in stream order, long before
  // any of them can wrap
  if (d->prog_epoch >= d->prog_epoch_limit) { HIPCHK(hipMemsetAsync(d->pctr, 0, (size_t)d->n_pctr * sizeof(int), st)); d->prog_epoch = 0; }
  const level_dev &l = d->prog;
  {
    scoped_timer t(d, st, 3, true);
    HIPCHK((hipError_t)chol_launch_program(d_arena, d->ws, d->jobs, d->n_job, d->pwaits, l.potrf, l.trsm, l.task, l.src, d->exts, d->pctr, d->pctr_total, d->prog_epoch,
                                           d->pctr + d->n_pctr - 1, d->prog_epoch * (d->n_job + d->prog_grid), d->prog_grid, info_cur, info_next, d->trace, st));
  }
  d->prog_epoch++;
  return 0;
}
extern "C" int cholamd_device_program_trace(cholamd_device *d, double *d_arena, void *stream, int64_t cap, int64_t *out, int *njobs_out)
{ // diagnostic: one program launch on d_arena with per-job stamps; out[5 j ..] = kind, drawn, waits over, ended (10 ns ticks since
  // the first job was drawn), workgroup
  HIPCHK(hipSetDevice(d->dev));
  if (!d->prog_ready) { chol_set_error("no program launch for this problem / these options"); return CHOLAMD_ERR_ARG; }
  *njobs_out = d->n_job;
  if (cap < (int64_t)5 * d->n_job) return 0;
  // 4 stamps per job, then CHOL_TRACE_X per job (chol_kernels.h)
  const size_t nst = (size_t)(4 + CHOL_TRACE_X) * d->n_job;
  std::vector<unsigned long long> h(nst);
  {
    dev_buf<unsigned long long> stamps;
    struct disarm { cholamd_device *d; ~disarm() { d->trace = nullptr; } } on_exit{ d }; // on every way out, before the stamps are released
    int rc = stamps.alloc_zero(nst);
    if (rc) return rc;
    d->trace = stamps;
    if ((rc = cholamd_factor(d, d_arena, stream))) return rc;
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(hipMemcpy(h.data(), stamps, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  }
  unsigned long long t0 = ~0ull;
  for (int j = 0; j < d->n_job; j++) if (h[4 * j] && h[4 * j] < t0) t0 = h[4 * j];
  for (int j = 0; j < d->n_job; j++) {
    out[5 * j] = d->jobs_host[j].kind + (d->jobs_host[j].kind == 0 && d->jobs_host[j].n_ext > 0 ? 10 : 0);
    for (int q = 0; q < 3; q++) out[5 * j + 1 + q] = (int64_t)(h[4 * j + q] - t0);
    out[5 * j + 4] = (int64_t)h[4 * j + 3];
  }
  if (const char *path = getenv("CHOLAMD_TRACE_FOLLOW")) { // diagnostic: the followers' per-item stamps as text (us since the first job was drawn)
    if (FILE *fp = fopen(path, "w")) {
      for (int j = 0; j < d->n_job; j++) {
        const unsigned long long *x = &h[(size_t)4 * d->n_job + (size_t)CHOL_TRACE_X * j];
        const int kind = d->jobs_host[j].kind;
        bool any = false;
        for (int i = 0; i < CHOL_TRACE_X; i++) any = any || x[i] != 0;
        if (!any) continue;
        if (kind == 2) { fprintf(fp, "job %d kind 2 last-stage-held %.1f\n", j, (double)(x[0] - t0) * 0.01); continue; } // update job: wave 0 saw its last staged wait hold
        fprintf(fp, "job %d kind %d", j, kind);
        if (kind == 0 && x[1]) {
          fprintf(fp, " items %llu own-tiles-wait-over %.1f rounds:", x[1], x[0] ? (double)(x[0] - t0) * 0.01 : -1.0);
          for (unsigned long long i = 0; i < x[1] && i < 44; i++) if (x[2 + i]) fprintf(fp, " %llu:%.1f", i, (double)(x[2 + i] - t0) * 0.01);
        }
        if (kind == 0 && x[24]) { fprintf(fp, " | prologue (entry, LDS init, tables, slot tables read, columns 0-1 requested, tiles requested, columns 0-1 parked):"); const int ord[7] = { 0, 1, 2, 5, 6, 3, 4 }; for (int k = 0; k < 7; k++) fprintf(fp, " %.1f", x[24 + ord[k]] ? (double)(x[24 + ord[k]] - t0) * 0.01 : -1.0); }
        fprintf(fp, kind == 0 ? " | column started:" : " | POTRF column seen:");
        for (int k = 0; k < 24; k++) if (x[72 + k]) fprintf(fp, " %d:%.1f", k, (double)(x[72 + k] - t0) * 0.01);
        fprintf(fp, kind == 0 ? " | column published:" : " | column tile on the channel:");
        for (int k = 0; k < 24; k++) if (x[48 + k]) fprintf(fp, " %d:%.1f", k, (double)(x[48 + k] - t0) * 0.01);
        fprintf(fp, "\n");
      }
      fclose(fp);
    }
  }
  return 0;
}
extern "C" int cholamd_factor_info(cholamd_device *d, int *sep_out)
{
  HIPCHK(hipSetDevice(d->dev));
  int h[2] = { 0, 0 };
  HIPCHK(hipMemcpy(h, d->info_last ? d->info_last : d->info, sizeof h, hipMemcpyDeviceToHost));
  if (sep_out) *sep_out = h[1];
  if (h[0] == CHOLAMD_ERR_STALL)
    chol_set_error("factorisation stalled: a workgroup of a fused launch waited ~50 ms for a progress word of the same launch and gave up; the factor is not valid");
  else if (h[0] < 0) chol_set_error("factorisation failed with internal code %d", h[0]);
  return h[0];
}

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
template <class TL> static int solve_any(cholamd_device *d, const TL *d_arena, const double *d_b, double *d_x, int which, hipStream_t st)
{
  if constexpr (std::is_same<TL, double>::value) { if (d->solve_reference_shape) return solve_reference(d, d_arena, d_b, d_x, which, st); }
  return solve_t(d, d_arena, d_b, d_x, which, st);
}
static int half_which_ok(int which, const char *what)
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

// ---------------------------------------------------------------------------------------------
// Mixed precision (BASELINE config 5): fp32 factor, fp64 iterative refinement of the solve.
// The fp32 arena has the element layout of the fp64 one (cholamd_plan_arena_doubles() floats).
// ---------------------------------------------------------------------------------------------
static void take_f32_verdict(cholamd_device *d, const int64_t *status)
{
  d->f32_range = status[0] == 0; d->f32_bad = status[0] ? status[1] : -1; d->f32_pending = false;
}
// the status words of the last (asynchronous) call, which are those of the values in force: one synchronisation of `st`
static int read_values_status(cholamd_device *d, hipStream_t st)
{
  HIPCHK(hipMemcpyAsync(d->vs_host, d->vs_dev, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::memcpy(d->vs_last, d->vs_host, sizeof d->vs_last);
  d->vs_last_valid = true;
  take_f32_verdict(d, d->vs_last);
  return 0;
}
// the fp32 factor converts A to float: an entry beyond FLT_MAX would become inf, one below FLT_MIN a denormal or zero, and the pivot checks do not see
// what that does to the factor.  Such a matrix is refused (include/cholamd.h); checked once per device object.
static int f32_range_ok(cholamd_device *d, hipStream_t st)
{
  const cholamd_plan *p = d->plan;
  if (d->vs_in_force) { // the values of cholamd_device_set_values: the verdict is in the status words of that call, read back once
    if (d->f32_pending) { int rc = read_values_status(d, st); if (rc) return rc; }
    if (d->f32_range) return 0;
    double v = 0.0; // the message names the value-array index; the value itself sits in the scatter list
    for (int64_t e = 0; e < p->nnz_a; e++)
      if (p->a_src[e] == d->f32_bad) { HIPCHK(hipMemcpy(&v, d->a_val + e, sizeof v, hipMemcpyDeviceToHost)); break; }
    chol_set_error("fp32 factor: entry %lld of A (%.17g) is outside the normal range of float [%g, %g]; use the fp64 factor", (long long)d->f32_bad,
                   v, (double)FLT_MIN, (double)FLT_MAX);
    return CHOLAMD_ERR_ARG;
  }
  if (d->f32_range < 0) {
    d->f32_range = 1;
    for (int64_t e = 0; e < p->nnz_a; e++) {
      const double a = std::fabs(p->a_val[e]);
      if (a > (double)FLT_MAX || a < (double)FLT_MIN) { d->f32_range = 0; d->f32_bad = e; break; } // (explicit zeros are not in a_val)
    }
  }
  if (d->f32_range) return 0;
  chol_set_error("fp32 factor: entry %lld of A (%.17g) is outside the normal range of float [%g, %g]; use the fp64 factor", (long long)d->f32_bad,
                 p->a_val[d->f32_bad], (double)FLT_MIN, (double)FLT_MAX);
  return CHOLAMD_ERR_ARG;
}
static int ensure_f32(cholamd_device *d, hipStream_t st)
{
  { int rc = f32_range_ok(d, st); if (rc) return rc; }
  { int rc = d->ws32.ensure((size_t)(d->plan->ws_doubles > 0 ? d->plan->ws_doubles : 1)); if (rc) return rc; }
  if (!d->lv32.empty()) return 0;
  const int L = d->plan->levels;
  chol_sched_opts o = d->opt;
  o.split_min = CHOL32_MAXN; o.split_nb = CHOL32_MAXN; o.fuse = 0; o.fuse_update_max = 0; o.trsm_group = CHOL32_TRSM_GROUP; // pivot blocks the LDS-resident fp32 POTRF takes, one launch per phase
  d->lv32.resize(L);
  for (int lvl = 0; lvl < L; lvl++) {
    chol_level_work w;
    int rc = chol_build_level_work(d->plan, &o, lvl, d->rank, d->world, &w);
    if (!rc) rc = upload_level(d->lv32[lvl], w, false); // the fp32 kernels have no role tables
    chol_level_work_free(&w);
    if (rc) { d->lv32.clear(); return rc; }
  }
  return 0;
}
static int ensure_csr(cholamd_device *d)
{ // the operator A alone (cholamd_apply needs no more).  csr_val is not uploaded twice: it follows cholamd_device_set_values
  const cholamd_plan *p = d->plan;
  const int n = p->n;
  const size_t ncsr = (size_t)(p->csr_ptr[n] > 0 ? p->csr_ptr[n] : 1);
  int rc = 0;
  if (!d->csr_ptr) rc = d->csr_ptr.upload(p->csr_ptr, (size_t)n + 1);
  if (!rc && !d->csr_col) rc = d->csr_col.upload(p->csr_col, ncsr);
  if (!rc && !d->csr_val) rc = d->csr_val.upload(p->csr_val, ncsr);
  return rc;
}
static int ensure_refine(cholamd_device *d)
{ // every buffer on its own: a call after a failure completes what is missing
  const int n = d->plan->n;
  int rc = ensure_csr(d);
  if (!rc) rc = d->rvec.ensure((size_t)n);
  if (!rc) rc = d->dxvec.ensure((size_t)n);
  if (!rc) rc = d->partial.ensure((size_t)2 * ((n + 255) / 256));
  return rc;
}
// ---------------------------------------------------------------------------------------------
// New values of A on the same pattern (include/cholamd.h at cholamd_device_set_values).  The copies of A's values a device object holds are the
// scatter list a_val (with the owned-top copies top_val cut from it) and the residual operator csr_val; k_set_values gathers both from the caller's
// value array through the plan's index lists, and counts what the values are.  No schedule, work list or solve list is touched (sched_gen stays).
// ---------------------------------------------------------------------------------------------
static int ensure_values(cholamd_device *d)
{
  if (d->vs_dev) return 0; // the last one allocated
  const cholamd_plan *p = d->plan;
  int rc = ensure_refine(d); // the residual operator follows the values from now on
  if (rc) return rc;
  const size_t ncsr = (size_t)p->csr_ptr[p->n];
  if (!d->a_src) rc = d->a_src.upload(p->a_src, (size_t)p->nnz_a);
  if (!rc && !d->csr_src) rc = d->csr_src.upload(p->csr_src, ncsr);
  if (!rc && !d->e_cls) rc = d->e_cls.upload(p->e_cls, (size_t)p->nz_file);
  const int64_t init[4] = { 0, INT64_MAX, 0, INT64_MAX };
  if (!rc && !d->vs_init) rc = d->vs_init.upload(init, (size_t)4);
  if (!rc) rc = d->vs_host.ensure(8);
  if (!rc) rc = d->vs_dev.alloc(4);
  return rc;
}
extern "C" int cholamd_device_set_values(cholamd_device *d, const double *d_vals, int64_t count, int flags, void *stream)
{
  const cholamd_plan *p = d->plan;
  if (!d_vals) { chol_set_error("cholamd_device_set_values: null value array"); return CHOLAMD_ERR_ARG; }
  if (count != p->nz_file) { chol_set_error("cholamd_device_set_values: value array of %lld entries, the plan has %d", (long long)count, p->nz_file); return CHOLAMD_ERR_ARG; }
  if (flags < 0 || (flags & ~CHOLAMD_VALUES_NOCHECK)) { chol_set_error("cholamd_device_set_values: bad flags %d", flags); return CHOLAMD_ERR_ARG; }
  HIPCHK(hipSetDevice(d->dev));
  { int rc = ensure_values(d); if (rc) return rc; }
  hipStream_t st = (hipStream_t)stream;
  const int64_t nz = p->nz_file, ncsr = p->csr_ptr[p->n];
  auto launch = [&](int parts) {
    return (hipError_t)chol_launch_set_values(d_vals, nz, d->e_cls, d->a_val, d->a_src, p->nnz_a, d->csr_val, d->csr_src, ncsr, parts, d->vs_dev, st);
  };
  if (flags & CHOLAMD_VALUES_NOCHECK) {
    HIPCHK(hipMemcpyAsync(d->vs_dev, d->vs_init, 4 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(launch(CHOL_VALUES_STATUS | CHOL_VALUES_GATHER));
    d->vs_last_valid = false; d->f32_range = -1; d->f32_pending = true;
  } else {
    // look first, gather afterwards: a refused array leaves every copy as it was.  The verdict on the values in force, if nobody has read it yet, is
    // taken along in the same synchronisation (the status words are about to be overwritten)
    const bool pending = d->f32_pending;
    if (pending) HIPCHK(hipMemcpyAsync(d->vs_host + 4, d->vs_dev, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(d->vs_dev, d->vs_init, 4 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(launch(CHOL_VALUES_STATUS));
    HIPCHK(hipMemcpyAsync(d->vs_host, d->vs_dev, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (pending) take_f32_verdict(d, d->vs_host + 4);
    std::memcpy(d->vs_last, d->vs_host, sizeof d->vs_last);
    d->vs_called = true; d->vs_last_valid = true;
    if (d->vs_last[2] > 0) {
      chol_set_error("cholamd_device_set_values: entry %lld of the value array is outside the pattern (0.0 when the plan was made) and %lld such entr%s not zero now; "
                     "the previous values stay in force (a new pattern needs a new plan)", (long long)d->vs_last[3], (long long)d->vs_last[2], d->vs_last[2] == 1 ? "y is" : "ies are");
      return CHOLAMD_ERR_ARG;
    }
    HIPCHK(launch(CHOL_VALUES_GATHER));
    take_f32_verdict(d, d->vs_last);
  }
  d->vs_called = true; d->vs_in_force = true;
  for (int q = 0; q < 2; q++) // the owned-top copies of the current schedule; a later rebuild (top_entries) gathers from a_val itself
    if (d->top_gen[q] == d->sched_gen && d->top_n[q] > 0) HIPCHK((hipError_t)chol_launch_gather(d->top_val[q], d->a_val, d->top_e[q], d->top_n[q], st));
  return 0;
}
extern "C" int cholamd_device_values_status(cholamd_device *d, void *stream, int64_t out[4])
{
  if (!d->vs_called) { chol_set_error("cholamd_device_values_status: no cholamd_device_set_values call on this device object yet"); return CHOLAMD_ERR_ARG; }
  HIPCHK(hipSetDevice(d->dev));
  if (!d->vs_last_valid) { int rc = read_values_status(d, (hipStream_t)stream); if (rc) return rc; }
  out[0] = d->vs_last[0]; out[1] = d->vs_last[0] ? d->vs_last[1] : -1;
  out[2] = d->vs_last[2]; out[3] = d->vs_last[2] ? d->vs_last[3] : -1;
  return 0;
}
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
static hipStream_t stream_of(void *const *streams, int g) { return streams ? (hipStream_t)streams[g] : nullptr; }
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
static int block_check(cholamd_device *d, bool with_arena, const void *arena, const double *B, int64_t ldb, const double *X, int64_t ldx, int nrhs, const char *what, const char *in,
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
template <class TL> static int solve_nrhs_any(cholamd_device *d, const TL *d_arena, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int cols, bool half, int which, hipStream_t st)
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

// ---------------------------------------------------------------------------------------------
// Multi-GPU: subtree sharding + ONE extend-add exchange over RCCL.
// The separator tree is cut at level d = log2(world): rank g owns the subtrees under its level-d separator and
// factors them locally; contributions to the shared top of the tree accumulate in the rank's own copy of the
// arena tail (the top panels are the contiguous tail of the arena: chol_plan.h); one ncclAllReduce(sum) over
// that tail is the exchange; the top levels follow on every rank.
// ---------------------------------------------------------------------------------------------
#define CHOL_LOCAL_MAX 64
extern "C" int cholamd_comm_unique_id(char id[CHOLAMD_UNIQUE_ID_BYTES])
{
  static_assert(sizeof(ncclUniqueId) <= CHOLAMD_UNIQUE_ID_BYTES, "unique id size");
  ncclUniqueId u;
  NCCLCHK(ncclGetUniqueId(&u));
  std::memset(id, 0, CHOLAMD_UNIQUE_ID_BYTES);
  std::memcpy(id, &u, sizeof u);
  return 0;
}
extern "C" int cholamd_comm_create(cholamd_device *d, int world, int rank, const char id[CHOLAMD_UNIQUE_ID_BYTES], cholamd_comm **out)
{
  *out = nullptr;
  if (world < 1 || rank < 0 || rank >= world) { chol_set_error("bad communicator rank %d of %d", rank, world); return CHOLAMD_ERR_ARG; }
  HIPCHK(hipSetDevice(d->dev));
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof u);
  cholamd_comm *c = new cholamd_comm();
  c->world = world; c->rank = rank;
  ncclResult_t r = ncclCommInitRank(&c->comm, world, u, rank);
  if (r != ncclSuccess) { chol_set_error("ncclCommInitRank failed: %s", ncclGetErrorString(r)); delete c; return CHOLAMD_ERR_COMM; }
  *out = c;
  return 0;
}
extern "C" int cholamd_comm_create_all(cholamd_device *const *devs, int n, cholamd_comm **out)
{ // one process driving n devices (cholamd_mmat --gpus n)
  if (n < 1) { chol_set_error("no devices"); return CHOLAMD_ERR_ARG; }
  std::vector<int> ids(n);
  std::vector<ncclComm_t> comms(n);
  for (int i = 0; i < n; i++) ids[i] = devs[i]->dev;
  NCCLCHK(ncclCommInitAll(comms.data(), n, ids.data()));
  for (int i = 0; i < n; i++) { out[i] = new cholamd_comm(); out[i]->comm = comms[i]; out[i]->world = n; out[i]->rank = i; }
  return 0;
}
extern "C" int cholamd_comm_create_local(cholamd_device *const *devs, int n, cholamd_comm **out)
{ // one process, n rank objects, no RCCL: device-side sums and peer copies (the ranks may share a device)
  if (n < 1 || n > CHOL_LOCAL_MAX) { chol_set_error("local communicator of %d ranks (1 .. %d)", n, CHOL_LOCAL_MAX); return CHOLAMD_ERR_ARG; }
  local_group *G = new local_group();
  G->n = n; G->refs = n; G->dev.resize(n); G->ev.resize(2 * n);
  for (int i = 0; i < n; i++) G->dev[i] = devs[i]->dev;
  for (int i = 0; i < n; i++) {
    HIPCHK(hipSetDevice(G->dev[i]));
    HIPCHK(hipEventCreateWithFlags(&G->ev[i], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&G->ev[n + i], hipEventDisableTiming));
    for (int j = 0; j < n; j++) if (G->dev[j] != G->dev[i]) {
      hipError_t e = hipDeviceEnablePeerAccess(G->dev[j], 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { chol_set_error("no peer access from device %d to device %d: %s", G->dev[i], G->dev[j], hipGetErrorString(e)); return CHOLAMD_ERR_COMM; }
      (void)hipGetLastError();
    }
  }
  for (int i = 0; i < n; i++) { out[i] = new cholamd_comm(); out[i]->world = n; out[i]->rank = i; out[i]->owned = false; out[i]->local = G; }
  return 0;
}
extern "C" int cholamd_comm_adopt(void *nccl_comm, int world, int rank, cholamd_comm **out)
{ // an ncclComm_t the caller made (and keeps): e.g. the one a Legion mapper or torch's process group holds
  if (!nccl_comm) { chol_set_error("null ncclComm_t"); return CHOLAMD_ERR_ARG; }
  cholamd_comm *c = new cholamd_comm();
  c->comm = (ncclComm_t)nccl_comm; c->world = world; c->rank = rank; c->owned = false;
  *out = c;
  return 0;
}
extern "C" int cholamd_comm_count(const cholamd_comm *c, int *ranks_out)
{ // ncclCommCount of the RCCL communicator behind the handle (a local communicator: its rank objects)
  if (!c) { chol_set_error("null communicator"); return CHOLAMD_ERR_ARG; }
  if (!c->comm) { *ranks_out = c->local ? c->local->n : 0; return 0; }
  int n = 0;
  NCCLCHK(ncclCommCount(c->comm, &n));
  *ranks_out = n;
  return 0;
}
extern "C" void cholamd_comm_destroy(cholamd_comm *c)
{
  if (!c) return;
  if (c->owned && c->comm) (void)ncclCommDestroy(c->comm);
  if (c->local && --c->local->refs == 0) {
    for (size_t i = 0; i < c->local->ev.size(); i++) { (void)hipSetDevice(c->local->dev[i % c->local->n]); (void)hipEventDestroy(c->local->ev[i]); }
    delete c->local;
  }
  delete c;
}
static int tail_of(const cholamd_device *d, int64_t *tail, int64_t *count)
{
  const cholamd_plan *p = d->plan;
  *tail = d->world > 1 ? p->panel_off[p->nsep - (d->world - 1) + 1] : p->arena;
  *count = p->arena - *tail;
  return 0;
}
extern "C" int64_t cholamd_device_tail_offset(const cholamd_device *d)
{
  int64_t t, c;
  tail_of(d, &t, &c);
  return t;
}
extern "C" int cholamd_comm_allreduce(cholamd_comm *c, double *d_buf, int64_t count, void *stream)
{ // in-place fp64 sum over the communicator's ranks, asynchronous on `stream` (of the current device)
  if (!c || !c->comm) { chol_set_error(c && c->local ? "a local communicator exchanges through cholamd_factor_multi only" : "null communicator"); return CHOLAMD_ERR_ARG; }
  if (count <= 0) return 0;
  NCCLCHK(ncclAllReduce(d_buf, d_buf, (size_t)count, ncclDouble, ncclSum, c->comm, (hipStream_t)stream));
  return 0;
}
static int comm_matches(const cholamd_device *d, const cholamd_comm *c)
{
  if (c && c->world == d->world && c->rank == d->rank) return 0;
  chol_set_error("communicator (rank %d of %d) does not match the device partition (rank %d of %d)", c ? c->rank : -1, c ? c->world : -1, d->rank, d->world);
  return CHOLAMD_ERR_ARG;
}
// ---- the extend-add exchange ------------------------------------------------------------------
// Replicated top levels: every rank needs the whole summed tail -> ONE in-place all-reduce.
// Top levels distributed by column blocks (option dist_top): after the exchange a rank works only on the column blocks it OWNS (it
// factors and solves them, applies the updates into them); every other block reaches it factored, by broadcast.  So the sum of a
// block is needed on its owner alone: every rank SENDS its partial copy of each block it does not own straight to the owner
// (grouped ncclSend / ncclRecv: point-to-point, all seven xGMI links of a GPU at once instead of a ring's one per direction), the
// owner adds the world - 1 copies it received to its own in RANK ORDER (deterministic: the same sum in every run).  A rank receives
// (world - 1) x (its owned blocks) and sends the blocks it does not own once: (world - 1) / world of the tail each way, against
// 2 (world - 1) / world of it each way for the ring all-reduce -- and nothing is added twice on the way.
// PATH-AWARE (round 4): a rank's subtree reaches only the top separators on its own path to the root (the reference touches a C tile only
// where the fill marks it, blas.rg:385-395, and the fill of a top block comes from the subtrees under it): its copy of every other
// top panel is zero -- unless it is rank 0, whose arena starts from A there.  So a rank SENDS only the blocks of the separators on its
// path (rank 0: all) and an owner RECEIVES only from the ranks under the block's separator and from rank 0 (chol_top_contributors);
// both ends compute the same lists from the plan, nothing about them travels.
struct xpiece { int64_t off, count, stage; int owner; unsigned contrib; };
// the column blocks of the levels above the cut, with their owners (the broadcast lists of the distributed top levels); empty: replicated
static void exchange_pieces(const cholamd_device *d, const std::vector<level_dev> &lv, std::vector<xpiece> &out)
{
  out.clear();
  const int split = chol_split_level(d->world);
  for (int lvl = split - 1; lvl >= 0 && lvl < (int)lv.size(); lvl--)
    for (const chol_bcast &b : lv[lvl].bcast) out.push_back({ b.off, b.count, 0, b.owner, chol_top_contributors(b.heap, d->world) });
  int64_t st = 0; // staging slots of the pieces this rank owns: one copy per contributing rank other than itself, senders in rank order
  for (xpiece &x : out) if (x.owner == d->rank) { x.stage = st; st += x.count * __builtin_popcount(x.contrib & ~(1u << d->rank)); }
}
// Multi-GPU: which entries of A a rank's fill scatters.  Everything under the cut on every rank (the panels of the other ranks' subtrees are
// never read).  The shared top of the tree (the tail of the arena) must start from A on exactly ONE rank per element, so that the sum over
// the ranks after the local levels is A_top - all contributions: with replicated top levels (one all-reduce of the tail) that is rank 0; with
// the top levels distributed by column blocks it is the block's OWNER -- the extend-add exchange then carries a block only from the ranks whose
// subtrees reach it (chol_top_contributors), and rank 0 sends no more than any other rank.  `*below` = leading entries of (a_dst, a_val) to
// scatter; (*tdst, *tval, *ntop) = further entries (device arrays).  f32: the fp32 schedule's column blocks.
static int top_entries(cholamd_device *d, int f32, int64_t *below, const int64_t **tdst, const double **tval, int64_t *ntop, hipStream_t st)
{
  const cholamd_plan *p = d->plan;
  *tdst = nullptr; *tval = nullptr; *ntop = 0;
  if (d->world <= 1) { *below = p->nnz_a; return 0; }
  const int64_t tail = p->panel_off[p->nsep - (d->world - 1) + 1];
  int64_t lo = 0, hi = p->nnz_a;
  while (lo < hi) { int64_t mid = (lo + hi) / 2; if (p->a_dst[mid] < tail) lo = mid + 1; else hi = mid; }
  *below = lo;
  if (d->top_gen[f32] != d->sched_gen) { // once per schedule
    d->top_dst[f32].reset(); d->top_val[f32].reset(); d->top_e[f32].reset(); d->top_n[f32] = 0;
    std::vector<xpiece> px;
    exchange_pieces(d, f32 ? d->lv32 : d->lv, px);
    if (px.empty()) d->top_n[f32] = d->rank == 0 ? -1 : 0; // replicated top levels: rank 0 scatters the whole tail
    else {
      std::vector<xpiece> mine;
      for (const xpiece &x : px) if (x.owner == d->rank) mine.push_back(x);
      std::sort(mine.begin(), mine.end(), [](const xpiece &a, const xpiece &b) { return a.off < b.off; });
      std::vector<int64_t> td; std::vector<int> te;
      size_t q = 0;
      for (int64_t e = lo; e < p->nnz_a; e++) { // a_dst ascends: one merge pass over the owned blocks
        while (q < mine.size() && mine[q].off + mine[q].count <= p->a_dst[e]) q++;
        if (q < mine.size() && p->a_dst[e] >= mine[q].off) { td.push_back(p->a_dst[e]); te.push_back((int)e); }
      }
      if (!td.empty()) {
        int rc = d->top_dst[f32].upload(td.data(), td.size());
        if (!rc) rc = d->top_e[f32].upload(te.data(), te.size());
        // the values: the device object's CURRENT ones (the plan's, or those of the last cholamd_device_set_values)
        if (!rc) rc = d->top_val[f32].alloc(td.size());
        if (rc) return rc;
        HIPCHK((hipError_t)chol_launch_gather(d->top_val[f32], d->a_val, d->top_e[f32], (int64_t)td.size(), st));
      }
      d->top_n[f32] = (int64_t)td.size();
    }
    d->top_gen[f32] = d->sched_gen;
  }
  if (d->top_n[f32] < 0) *below = p->nnz_a;
  else { *tdst = d->top_dst[f32]; *tval = d->top_val[f32]; *ntop = d->top_n[f32]; }
  return 0;
}
template <class T> __global__ void k_sum_owned(T *arena, const T *stage, const sum_desc *desc, int world, int rank)
{ // arena[off + i] = sum over the ranks in rank order; rank r's copy: this rank's own arena for r == rank, else -- if r contributes -- the next staging slot
  const sum_desc d = desc[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.count; i += (int64_t)gridDim.x * blockDim.x) {
    T s = 0;
    int slot = 0;
    for (int r = 0; r < world; r++) {
      if (r == rank) s += arena[d.off + i];
      else if (d.contrib & (1u << r)) { s += stage[d.stage + (int64_t)slot * d.count + i]; slot++; }
    }
    arena[d.off + i] = s;
  }
}
// The rank-ordered sum of what exchange_owned() received: it must reach the stream AFTER the sends and receives, and those reach it only
// when the OUTERMOST RCCL group ends -- a caller that groups the exchanges of several ranks (factor_multi_t) posts them all with
// `defer_sum` and calls this once its group has ended.
template <class T> static int exchange_owned_sum(cholamd_device *d, T *arena, const std::vector<xpiece> &px, hipStream_t st)
{
  int64_t mx = 0; unsigned mine = 0;
  for (const xpiece &x : px) if (x.owner == d->rank) { mx = x.count > mx ? x.count : mx; mine++; }
  if (!mine) return 0;
  HIPCHK(hipSetDevice(d->dev));
  const int64_t bx = (mx + 255) / 256;
  hipLaunchKernelGGL(k_sum_owned<T>, dim3((unsigned)(bx < 1024 ? bx : 1024), mine), dim3(256), 0, st, arena, (const T *)d->xstage.get(), d->xdesc.get(), d->world, d->rank);
  HIPCHK(hipGetLastError());
  return 0;
}
template <class T> static int exchange_owned(cholamd_device *d, T *arena, const std::vector<xpiece> &px, cholamd_comm *c, hipStream_t st, bool defer_sum)
{
  const ncclDataType_t ty = sizeof(T) == 8 ? ncclDouble : ncclFloat;
  int64_t need = 0; std::vector<sum_desc> mine;
  for (const xpiece &x : px) if (x.owner == d->rank) { need += x.count * __builtin_popcount(x.contrib & ~(1u << d->rank)); mine.push_back({ x.off, x.count, x.stage, x.contrib, 0 }); }
  if ((size_t)need * sizeof(T) > d->xstage_bytes) {
    HIPCHK(hipStreamSynchronize(st));
    d->xstage_bytes = 0;
    { int rc = d->xstage.alloc_bytes((size_t)need * sizeof(T), 1); if (rc) return rc; }
    d->xstage_bytes = (size_t)need * sizeof(T);
  }
  if (d->xdesc_gen != d->sched_gen || d->xdesc_elem != (int)sizeof(T)) { // the descriptors of the sum kernel, once per schedule
    HIPCHK(hipStreamSynchronize(st));
    { int rc = d->xdesc.upload(mine.data(), mine.size()); if (rc) return rc; }
    d->xdesc_gen = d->sched_gen; d->xdesc_elem = (int)sizeof(T);
  }
  T *stage = (T *)d->xstage.get();
  NCCLCHK(ncclGroupStart());
  for (const xpiece &x : px) {
    ncclResult_t r = ncclSuccess;
    if (x.owner == d->rank) {
      for (int q = 0, slot = 0; q < d->world && r == ncclSuccess; q++) {
        if (q == d->rank || !(x.contrib & (1u << q))) continue;
        r = ncclRecv(stage + x.stage + (int64_t)slot * x.count, (size_t)x.count, ty, q, c->comm, st);
        slot++;
      }
    } else if (x.contrib & (1u << d->rank)) r = ncclSend(arena + x.off, (size_t)x.count, ty, x.owner, c->comm, st);
    if (r != ncclSuccess) { (void)ncclGroupEnd(); chol_set_error("ncclSend/ncclRecv failed: %s", ncclGetErrorString(r)); return CHOLAMD_ERR_COMM; }
  }
  NCCLCHK(ncclGroupEnd());
  return defer_sum ? 0 : exchange_owned_sum<T>(d, arena, px, st);
}
// defer_sum: the caller holds an RCCL group open around this call and runs exchange_sum_t() after closing it
template <class T> static int exchange_tail_t(cholamd_device *d, T *arena, const std::vector<level_dev> &lv, cholamd_comm *c, hipStream_t st, bool defer_sum = false)
{
  HIPCHK(hipSetDevice(d->dev));
  if (comm_matches(d, c)) return CHOLAMD_ERR_ARG;
  if (!c->comm) { chol_set_error("a local communicator exchanges through cholamd_factor_multi only"); return CHOLAMD_ERR_ARG; }
  std::vector<xpiece> px;
  exchange_pieces(d, lv, px);
  if (!px.empty()) return exchange_owned<T>(d, arena, px, c, st, defer_sum);
  int64_t tail, count;
  tail_of(d, &tail, &count);
  if (count <= 0) return 0;
  NCCLCHK(ncclAllReduce(arena + tail, arena + tail, (size_t)count, sizeof(T) == 8 ? ncclDouble : ncclFloat, ncclSum, c->comm, st));
  return 0;
}
template <class T> static int exchange_sum_t(cholamd_device *d, T *arena, const std::vector<level_dev> &lv, hipStream_t st)
{ // second half of exchange_tail_t(..., defer_sum = true)
  std::vector<xpiece> px;
  exchange_pieces(d, lv, px);
  return px.empty() ? 0 : exchange_owned_sum<T>(d, arena, px, st);
}
extern "C" int cholamd_exchange_tail(cholamd_device *d, double *d_arena, cholamd_comm *c, void *stream)
{
  return exchange_tail_t<double>(d, d_arena, d->lv, c, (hipStream_t)stream);
}
extern "C" int cholamd_exchange_volume(const cholamd_device *d, int64_t out[4])
{ // elements this rank receives / sends in the exchange of its partition, elements of the tail, pieces (0: one all-reduce of the tail:
  // a ring moves 2 (world - 1) / world of it each way)
  std::vector<xpiece> px;
  exchange_pieces(d, d->lv, px);
  int64_t tail, count;
  tail_of(d, &tail, &count);
  out[0] = out[1] = 0; out[2] = count; out[3] = (int64_t)px.size();
  for (const xpiece &x : px) { if (x.owner == d->rank) out[0] += x.count * __builtin_popcount(x.contrib & ~(1u << d->rank)); else if (x.contrib & (1u << d->rank)) out[1] += x.count; }
  if (px.empty() && d->world > 1) out[0] = out[1] = 2 * count * (d->world - 1) / d->world;
  return 0;
}
// one rank's broadcasts of a CHOL_PH_BCAST phase (distributed top levels): every column block of the step travels from its owner to all
// ranks, in place at the same arena offset; one RCCL group
template <class T> static int bcast_rank_t(cholamd_device *d, const level_dev &l, const chol_phase &ph, T *d_arena, cholamd_comm *c, hipStream_t st)
{
  if (!c) { chol_set_error("the distributed top levels (option dist_top) need a communicator: cholamd_factor_sharded / cholamd_factor_multi"); return CHOLAMD_ERR_ARG; }
  if (comm_matches(d, c)) return CHOLAMD_ERR_ARG;
  if (!c->comm) { chol_set_error("a local communicator exchanges through cholamd_factor_multi only"); return CHOLAMD_ERR_ARG; }
  NCCLCHK(ncclGroupStart());
  for (int i = ph.first; i < ph.first + ph.n; i++) {
    const chol_bcast &b = l.bcast[i];
    ncclResult_t r = ncclBroadcast(d_arena + b.off, d_arena + b.off, (size_t)b.count, sizeof(T) == 8 ? ncclDouble : ncclFloat, b.owner, c->comm, st);
    if (r != ncclSuccess) { (void)ncclGroupEnd(); chol_set_error("ncclBroadcast failed: %s", ncclGetErrorString(r)); return CHOLAMD_ERR_COMM; }
  }
  NCCLCHK(ncclGroupEnd());
  return 0;
}
// ---- the level-by-level factor, written once for both element types of the arena ----
// T = double: the fp64 schedule (lv) and workspace; T = float: the fp32 ones, which ensure_f32 builds at the first call that needs them
template <class T> static const std::vector<level_dev> &levels_of(const cholamd_device *d) { if constexpr (sizeof(T) == 4) return d->lv32; else return d->lv; }
template <class T> static T *ws_of(const cholamd_device *d) { if constexpr (sizeof(T) == 4) return d->ws32; else return d->ws; }
template <class T> static int device_fill(cholamd_device *d, T *d_arena, hipStream_t st)
{
  constexpr bool F32 = sizeof(T) == 4;
  HIPCHK(hipSetDevice(d->dev));
  if constexpr (F32) { int rc = ensure_f32(d, st); if (rc) return rc; } // the fp32 schedule's column blocks decide which entries of the shared top are this rank's
  { int rc = clear_owned(d, d_arena, sizeof(T), st); if (rc) return rc; }
  int64_t below = 0, ntop = 0; const int64_t *tdst = nullptr; const double *tval = nullptr;
  { int rc = top_entries(d, F32, &below, &tdst, &tval, &ntop, st); if (rc) return rc; }
  HIPCHK((hipError_t)chol_launch_scatter(d_arena, d->a_dst, d->a_val, below, st));
  if (ntop > 0) HIPCHK((hipError_t)chol_launch_scatter(d_arena, tdst, tval, ntop, st));
  return 0;
}
extern "C" int cholamd_device_fill(cholamd_device *d, double *d_arena, void *stream) { return device_fill(d, d_arena, (hipStream_t)stream); }
extern "C" int cholamd_device_fill_f32(cholamd_device *d, float *d_arena32, void *stream) { return device_fill(d, d_arena32, (hipStream_t)stream); }
// the timing kind (cholamd_device_get_timing) a phase's launch is booked under: 0 potrf (+ fused trsm), 1 trsm, 2 update
static int timing_kind_of(int phase_kind)
{
  switch (phase_kind) {
    case CHOL_PH_POTRF: case CHOL_PH_FUSED: return 0;
    case CHOL_PH_TRSM: case CHOL_PH_TRSM_W: case CHOL_PH_TRSM_WT: return 1;
    default: return 2; // CHOL_PH_UPDATE, CHOL_PH_UPDATE_MT
  }
}
template <class T> static int launch_phase(cholamd_device *d, const level_dev &l, const chol_phase &ph, T *d_arena, hipStream_t st)
{
  constexpr bool F32 = sizeof(T) == 4;
  T *const ws = ws_of<T>(d);
  const int kind = F32 && ph.kind == CHOL_PH_TRSM_W ? CHOL_PH_TRSM : ph.kind; // the one-wave strips are an fp64 kernel: the fp32 factor takes them like CHOL_PH_TRSM
  if (kind == CHOL_PH_POTRF) HIPCHK((hipError_t)chol_launch_potrf(d_arena, ws, l.potrf + ph.first, ph.n, d->info, st));
  else if (kind == CHOL_PH_TRSM) HIPCHK((hipError_t)chol_launch_trsm(d_arena, ws, l.trsm + ph.first, ph.n, st));
  else if (kind == CHOL_PH_TRSM_WT) HIPCHK((hipError_t)chol_launch_trsm_wt(d_arena, ws, l.trsm + ph.first, ph.n, st));
  else if (kind == CHOL_PH_UPDATE) HIPCHK((hipError_t)chol_launch_update(d_arena, l.task + ph.first, l.src, ph.n, st));
  else if (kind == CHOL_PH_UPDATE_MT) HIPCHK((hipError_t)chol_launch_update_mt(d_arena, l.task_mt + ph.first, l.src, ph.n, (int64_t)d->plan->arena, st));
  else if constexpr (F32) { chol_set_error("internal: phase kind %d in the fp32 schedule", ph.kind); return CHOLAMD_ERR_ARG; }
  else if (kind == CHOL_PH_TRSM_W) HIPCHK((hipError_t)chol_launch_trsm_w(d_arena, ws, l.trsm + ph.first, ph.n, st));
  else if (kind == CHOL_PH_FUSED) { // the fused launch (fp64 only)
    // the progress words (epoch * 64 + columns) and the count of finished TRSM workgroups are monotonic across launches:
    // both start over, in stream order, long before either can wrap
    if (d->epoch >= (1 << 24) || d->done_total >= (1 << 30)) { HIPCHK(hipMemsetAsync(d->progress, 0, (size_t)(d->plan->nsep + 2) * sizeof(int), st)); d->epoch = 0; d->done_total = 0; }
    d->epoch++;
    if (ph.n3 > 0) d->done_total += (ph.n2 + 2) / 3; // TRSM workgroups of this launch count themselves out only when update tasks ride along
    HIPCHK((hipError_t)chol_launch_potrf_trsm(d_arena, ws, l.potrf + ph.first, ph.n, l.trsm + ph.first2, ph.n2, l.task + ph.first3, l.src, ph.n3,
                                              d->info, d->progress, d->epoch * 64, d->progress + d->plan->nsep + 1, d->done_total, st));
  }
  return 0;
}
// levels [level_lo, level_hi] of one rank; a broadcast phase (CHOL_PH_BCAST: distributed top levels: the step's column blocks travel from their owners to every
// rank) goes through `c`
template <class T> static int factor_levels_comm(cholamd_device *d, T *d_arena, int level_hi, int level_lo, cholamd_comm *c, hipStream_t st)
{
  HIPCHK(hipSetDevice(d->dev));
  if constexpr (sizeof(T) == 4) { int rc = ensure_f32(d, st); if (rc) return rc; }
  const int L = d->plan->levels;
  if (level_hi >= L) level_hi = L - 1;
  if (level_lo < 0) level_lo = 0;
  if (level_hi == L - 1) HIPCHK(hipMemsetAsync(d->info, 0, 2 * sizeof(int), st));
  d->info_last = d->info; d->info_foreign = true; // slot 0: the level-by-level paths
  for (int lvl = level_hi; lvl >= level_lo; lvl--) { // mmat.rg:1227
    const level_dev &l = levels_of<T>(d)[lvl];
    for (const chol_phase &ph : l.phase) {
      if (ph.kind == CHOL_PH_BCAST) {
        scoped_timer t(d, st, CHOL_TK_BCAST, ph.n > 0);
        int rc = bcast_rank_t<T>(d, l, ph, d_arena, c, st);
        if (rc) return rc;
        continue;
      }
      scoped_timer t(d, st, timing_kind_of(ph.kind), ph.n > 0);
      int rc = launch_phase<T>(d, l, ph, d_arena, st);
      if (rc) return rc;
    }
  }
  return 0;
}
extern "C" int cholamd_factor_levels(cholamd_device *d, double *d_arena, int level_hi, int level_lo, void *stream)
{ return factor_levels_comm(d, d_arena, level_hi, level_lo, nullptr, (hipStream_t)stream); }
extern "C" int cholamd_factor_levels_f32(cholamd_device *d, float *d_arena32, int level_hi, int level_lo, void *stream)
{ return factor_levels_comm(d, d_arena32, level_hi, level_lo, nullptr, (hipStream_t)stream); }
extern "C" int cholamd_factor_f32(cholamd_device *d, float *d_arena32, void *stream) { return cholamd_factor_levels_f32(d, d_arena32, d->plan->levels - 1, 0, stream); }
// one rank of a sharded factorisation: its subtrees' levels, the extend-add exchange of the shared top, the top levels.  The fp32 factor (BASELINE config 5:
// mixed precision x multi-GPU): an fp32 arena of the fp64 arena's element layout, the fp32 schedule partitioned like the fp64 one, the exchange and the
// broadcasts on floats
template <class T> static int factor_sharded(cholamd_device *d, T *d_arena, cholamd_comm *c, hipStream_t st)
{
  const int L = d->plan->levels, split = chol_split_level(d->world);
  if (d->world == 1) { if constexpr (sizeof(T) == 4) return cholamd_factor_f32(d, d_arena, st); else return cholamd_factor(d, d_arena, st); } // (fp64: the program launch)
  int rc = factor_levels_comm(d, d_arena, L - 1, split, nullptr, st);
  if (!rc) {
    scoped_timer t(d, st, CHOL_TK_EXCHANGE, true);
    rc = exchange_tail_t<T>(d, d_arena, levels_of<T>(d), c, st);
  }
  if (!rc) rc = factor_levels_comm(d, d_arena, split - 1, 0, c, st);
  return rc;
}
extern "C" int cholamd_factor_sharded(cholamd_device *d, double *d_arena, cholamd_comm *c, void *stream) { return factor_sharded(d, d_arena, c, (hipStream_t)stream); }
extern "C" int cholamd_factor_sharded_f32(cholamd_device *d, float *d_arena32, cholamd_comm *c, void *stream) { return factor_sharded(d, d_arena32, c, (hipStream_t)stream); }

// ---- one process driving n ranks ----
struct ptr_pack { void *p[CHOL_LOCAL_MAX]; };
template <class T> __global__ void k_sum_ranks(ptr_pack P, int n, T *dst, int64_t count)
{ // dst[i] = sum over the n copies in the order of the pack (rank order: run-to-run identical); dst may be one of them
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    T s = ((const T *)P.p[0])[i];
    for (int r = 1; r < n; r++) s += ((const T *)P.p[r])[i];
    dst[i] = s;
  }
}
template <class T> static int local_exchange(cholamd_device *const *devs, T *const *arenas, const std::vector<level_dev> &lv0, local_group *G, int n, void *const *streams)
{
  std::vector<xpiece> px;
  exchange_pieces(devs[0], lv0, px);
  int64_t tail, count;
  tail_of(devs[0], &tail, &count);
  if (count <= 0) return 0;
  for (int g = 0; g < n; g++) { HIPCHK(hipSetDevice(devs[g]->dev)); HIPCHK(hipEventRecord(G->ev[g], stream_of(streams, g))); } // every rank's subtree levels are in its stream
  if (px.empty()) { // replicated top: the ordered sum on rank 0, peer copies to the others
    HIPCHK(hipSetDevice(devs[0]->dev));
    ptr_pack P;
    for (int g = 0; g < n; g++) { P.p[g] = arenas[g] + tail; if (g) HIPCHK(hipStreamWaitEvent(stream_of(streams, 0), G->ev[g], 0)); }
    const int64_t blocks = (count + 255) / 256;
    hipLaunchKernelGGL(k_sum_ranks<T>, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream_of(streams, 0), P, n, arenas[0] + tail, count);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(G->ev[n], stream_of(streams, 0)));
    for (int g = 1; g < n; g++) {
      HIPCHK(hipSetDevice(devs[g]->dev));
      HIPCHK(hipStreamWaitEvent(stream_of(streams, g), G->ev[n], 0));
      HIPCHK(hipMemcpyPeerAsync(arenas[g] + tail, devs[g]->dev, arenas[0] + tail, devs[0]->dev, (size_t)count * sizeof(T), stream_of(streams, g)));
      HIPCHK(hipEventRecord(G->ev[n + g], stream_of(streams, g)));
    }
    HIPCHK(hipSetDevice(devs[0]->dev));
    for (int g = 1; g < n; g++) HIPCHK(hipStreamWaitEvent(stream_of(streams, 0), G->ev[n + g], 0)); // rank 0 goes on writing its tail
    return 0;
  }
  // distributed top: every column block is summed (rank order) into its OWNER's arena by the owner's stream; the other ranks' copies of
  // it are read, not written.  Nobody goes on before every owner has read what it needs (the broadcasts overwrite those copies)
  for (int o = 0; o < n; o++) {
    HIPCHK(hipSetDevice(devs[o]->dev));
    for (int g = 0; g < n; g++) if (g != o) HIPCHK(hipStreamWaitEvent(stream_of(streams, o), G->ev[g], 0));
    for (const xpiece &x : px) {
      if (x.owner != o) continue;
      ptr_pack P; // the copies that can be non-zero (the same set the RCCL path sends) and the owner's own, in rank order
      int np = 0;
      for (int g = 0; g < n; g++) if (g == o || (x.contrib & (1u << g))) P.p[np++] = arenas[g] + x.off;
      const int64_t blocks = (x.count + 255) / 256;
      hipLaunchKernelGGL(k_sum_ranks<T>, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, stream_of(streams, o), P, np, arenas[o] + x.off, x.count);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(G->ev[n + o], stream_of(streams, o)));
  }
  for (int g = 0; g < n; g++) {
    HIPCHK(hipSetDevice(devs[g]->dev));
    for (int o = 0; o < n; o++) if (o != g) HIPCHK(hipStreamWaitEvent(stream_of(streams, g), G->ev[n + o], 0));
  }
  return 0;
}
template <class T> static int local_bcast(cholamd_device *const *devs, T *const *arenas, local_group *G, int n, void *const *streams, const level_dev &l, const chol_phase &ph)
{
  std::vector<char> owner_ready(n, 0);
  for (int i = ph.first; i < ph.first + ph.n; i++) {
    const int o = l.bcast[i].owner;
    if (owner_ready[o]) continue;
    owner_ready[o] = 1;
    HIPCHK(hipSetDevice(devs[o]->dev));
    HIPCHK(hipEventRecord(G->ev[o], stream_of(streams, o))); // the owner's POTRF + TRSM of the step are in its stream
  }
  for (int g = 0; g < n; g++) {
    HIPCHK(hipSetDevice(devs[g]->dev));
    for (int o = 0; o < n; o++) if (owner_ready[o] && o != g) HIPCHK(hipStreamWaitEvent(stream_of(streams, g), G->ev[o], 0));
    for (int i = ph.first; i < ph.first + ph.n; i++) {
      const chol_bcast &b = l.bcast[i];
      if (b.owner == g) continue; // the owner does not touch the block again: the copies may read it while its stream goes on
      HIPCHK(hipMemcpyPeerAsync(arenas[g] + b.off, devs[g]->dev, arenas[b.owner] + b.off, devs[b.owner]->dev, (size_t)b.count * sizeof(T), stream_of(streams, g)));
    }
  }
  return 0;
}
// T = double: the fp64 schedule (devs[g]->lv); T = float: the fp32 one (lv32)
template <class T> static int factor_multi_t(cholamd_device *const *devs, T *const *arenas, cholamd_comm *const *comms, int n, void *const *streams)
{ // one process, n ranks: everything is asynchronous on each rank's stream
  constexpr bool F32 = sizeof(T) == 4;
  if (n < 1) { chol_set_error("no devices"); return CHOLAMD_ERR_ARG; }
  const int L = devs[0]->plan->levels, split = chol_split_level(n);
  local_group *G = comms[0] ? comms[0]->local : nullptr;
  for (int g = 0; g < n; g++) {
    if (devs[g]->world != n || devs[g]->rank != g) { chol_set_error("device %d is not partitioned as rank %d of %d", g, g, n); return CHOLAMD_ERR_ARG; }
    if (comm_matches(devs[g], comms[g])) return CHOLAMD_ERR_ARG;
    if (comms[g]->local != G || (!G && !comms[g]->comm)) { chol_set_error("the %d communicators are not of one kind", n); return CHOLAMD_ERR_ARG; }
    int rc = factor_levels_comm(devs[g], arenas[g], L - 1, split, nullptr, stream_of(streams, g));
    if (rc) return rc;
  }
  if (G) { int rc = local_exchange<T>(devs, arenas, levels_of<T>(devs[0]), G, n, streams); if (rc) return rc; }
  else {
    NCCLCHK(ncclGroupStart());
    for (int g = 0; g < n; g++) {
      int rc = exchange_tail_t<T>(devs[g], arenas[g], levels_of<T>(devs[g]), comms[g], stream_of(streams, g), true);
      if (rc) { (void)ncclGroupEnd(); return rc; }
    }
    NCCLCHK(ncclGroupEnd());
    // the owners' sums go behind the sends and receives, which entered the streams only now (the end of the outermost group)
    for (int g = 0; g < n; g++) { int rc = exchange_sum_t<T>(devs[g], arenas[g], levels_of<T>(devs[g]), stream_of(streams, g)); if (rc) return rc; }
  }
  // top levels: every rank runs its phases up to its next broadcast phase; the broadcasts of all ranks form one group
  for (int lvl = split - 1; lvl >= 0; lvl--) {
    std::vector<size_t> cur(n, 0);
    for (;;) {
      int at_bcast = 0;
      for (int g = 0; g < n; g++) {
        const level_dev &l = levels_of<T>(devs[g])[lvl];
        HIPCHK(hipSetDevice(devs[g]->dev));
        while (cur[g] < l.phase.size() && l.phase[cur[g]].kind != CHOL_PH_BCAST) {
          int rc = launch_phase(devs[g], l, l.phase[cur[g]], arenas[g], stream_of(streams, g));
          if (rc) return rc;
          cur[g]++;
        }
        if (cur[g] < l.phase.size()) at_bcast++;
      }
      if (at_bcast == 0) break;
      if (at_bcast != n) { chol_set_error("internal: the ranks disagree on the broadcast sequence of level %d", lvl); return CHOLAMD_ERR_ARG; }
      if (G) { int rc = local_bcast<T>(devs, arenas, G, n, streams, levels_of<T>(devs[0])[lvl], levels_of<T>(devs[0])[lvl].phase[cur[0]]); if (rc) return rc; }
      else {
        NCCLCHK(ncclGroupStart());
        for (int g = 0; g < n; g++) {
          const level_dev &l = levels_of<T>(devs[g])[lvl];
          const chol_phase &ph = l.phase[cur[g]];
          for (int i = ph.first; i < ph.first + ph.n; i++) {
            const chol_bcast &b = l.bcast[i];
            ncclResult_t r = ncclBroadcast(arenas[g] + b.off, arenas[g] + b.off, (size_t)b.count, F32 ? ncclFloat : ncclDouble, b.owner, comms[g]->comm, stream_of(streams, g));
            if (r != ncclSuccess) { (void)ncclGroupEnd(); chol_set_error("ncclBroadcast failed: %s", ncclGetErrorString(r)); return CHOLAMD_ERR_COMM; }
          }
        }
        NCCLCHK(ncclGroupEnd());
      }
      for (int g = 0; g < n; g++) cur[g]++;
    }
  }
  return 0;
}
extern "C" int cholamd_factor_multi(cholamd_device *const *devs, double *const *arenas, cholamd_comm *const *comms, int n, void *const *streams)
{
  if (n == 1) return cholamd_factor(devs[0], arenas[0], streams ? streams[0] : nullptr);
  return factor_multi_t<double>(devs, arenas, comms, n, streams);
}
extern "C" int cholamd_factor_multi_f32(cholamd_device *const *devs, float *const *arenas32, cholamd_comm *const *comms, int n, void *const *streams)
{
  if (n == 1) return cholamd_factor_f32(devs[0], arenas32[0], streams ? streams[0] : nullptr);
  return factor_multi_t<float>(devs, arenas32, comms, n, streams);
}
// one rank's part of the gather: the panels of the subtrees it owns travel to rank 0 (grouped ncclSend / ncclRecv), whose arena then
// holds the complete factor (for the solve / refinement and the writers).  elem_bytes = 8 (fp64 arena) or 4 (fp32)
extern "C" int cholamd_gather_to_root(cholamd_device *d, void *d_arena, int elem_bytes, cholamd_comm *c, void *stream)
{
  HIPCHK(hipSetDevice(d->dev));
  if (d->world == 1) return 0;
  if (comm_matches(d, c)) return CHOLAMD_ERR_ARG;
  if (!c->comm) { chol_set_error("a local communicator gathers through cholamd_gather_factor only"); return CHOLAMD_ERR_ARG; }
  if (elem_bytes != 4 && elem_bytes != 8) { chol_set_error("element size %d", elem_bytes); return CHOLAMD_ERR_ARG; }
  const cholamd_plan *p = d->plan;
  NCCLCHK(ncclGroupStart());
  for (int s = 1; s <= p->nsep; s++) {
    const int g = chol_owner_of(p, s, d->world);
    if (g <= 0 || (d->rank != 0 && d->rank != g)) continue;
    const int64_t off = p->panel_off[s], len = (s < p->nsep ? p->panel_off[s + 1] : p->arena) - off;
    char *ptr = (char *)d_arena + (size_t)off * elem_bytes;
    ncclResult_t r = d->rank == 0 ? ncclRecv(ptr, (size_t)len, elem_bytes == 8 ? ncclDouble : ncclFloat, g, c->comm, (hipStream_t)stream)
                                  : ncclSend(ptr, (size_t)len, elem_bytes == 8 ? ncclDouble : ncclFloat, 0, c->comm, (hipStream_t)stream);
    if (r != ncclSuccess) { (void)ncclGroupEnd(); chol_set_error("gather: %s", ncclGetErrorString(r)); return CHOLAMD_ERR_COMM; }
  }
  NCCLCHK(ncclGroupEnd());
  return 0;
}
static int gather_factor_bytes(cholamd_device *const *devs, void *const *arenas, int n, void *const *streams, int elem_bytes)
{ // the panels of the subtrees ranks 1..n-1 own -> device 0's arena (peer copies), so that it holds the complete factor
  const cholamd_plan *p = devs[0]->plan;
  for (int g = 1; g < n; g++) {
    HIPCHK(hipSetDevice(devs[g]->dev));
    HIPCHK(hipStreamSynchronize(streams ? (hipStream_t)streams[g] : nullptr));
  }
  HIPCHK(hipSetDevice(devs[0]->dev));
  for (int s = 1; s <= p->nsep; s++) {
    const int g = chol_owner_of(p, s, n);
    if (g <= 0) continue;
    const int64_t off = p->panel_off[s];
    const int64_t len = (s < p->nsep ? p->panel_off[s + 1] : p->arena) - off;
    HIPCHK(hipMemcpyPeerAsync((char *)arenas[0] + (size_t)off * elem_bytes, devs[0]->dev, (const char *)arenas[g] + (size_t)off * elem_bytes, devs[g]->dev, (size_t)len * elem_bytes, streams ? (hipStream_t)streams[0] : nullptr));
  }
  return 0;
}
extern "C" int cholamd_gather_factor(cholamd_device *const *devs, double *const *arenas, int n, void *const *streams)
{
  return gather_factor_bytes(devs, (void *const *)arenas, n, streams, 8);
}
extern "C" int cholamd_gather_factor_f32(cholamd_device *const *devs, float *const *arenas32, int n, void *const *streams)
{
  return gather_factor_bytes(devs, (void *const *)arenas32, n, streams, 4);
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
// one process driving n ranks: the two sums as an ordered device-side sum on rank 0's stream and peer copies back (local communicator), or grouped
// ncclAllReduce calls (cholamd_comm_create_all)
static int multi_sum_vec(cholamd_device *const *devs, cholamd_comm *const *comms, int n, void *const *streams, int64_t off, int64_t count)
{ // devs[g]->ytmp[off, off + count) <- sum over the ranks, on every rank
  if (count <= 0) return 0;
  local_group *G = comms[0]->local;
  if (!G) {
    NCCLCHK(ncclGroupStart());
    for (int g = 0; g < n; g++) {
      ncclResult_t r = ncclAllReduce(devs[g]->ytmp + off, devs[g]->ytmp + off, (size_t)count, ncclDouble, ncclSum, comms[g]->comm, stream_of(streams, g));
      if (r != ncclSuccess) { (void)ncclGroupEnd(); chol_set_error("ncclAllReduce failed: %s", ncclGetErrorString(r)); return CHOLAMD_ERR_COMM; }
    }
    NCCLCHK(ncclGroupEnd());
    return 0;
  }
  for (int g = 0; g < n; g++) { HIPCHK(hipSetDevice(devs[g]->dev)); HIPCHK(hipEventRecord(G->ev[g], stream_of(streams, g))); }
  HIPCHK(hipSetDevice(devs[0]->dev));
  ptr_pack P;
  for (int g = 0; g < n; g++) { P.p[g] = devs[g]->ytmp + off; if (g) HIPCHK(hipStreamWaitEvent(stream_of(streams, 0), G->ev[g], 0)); }
  const int64_t blocks = (count + 255) / 256;
  hipLaunchKernelGGL(k_sum_ranks<double>, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, stream_of(streams, 0), P, n, devs[0]->ytmp + off, count);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(G->ev[n], stream_of(streams, 0)));
  for (int g = 1; g < n; g++) {
    HIPCHK(hipSetDevice(devs[g]->dev));
    HIPCHK(hipStreamWaitEvent(stream_of(streams, g), G->ev[n], 0));
    HIPCHK(hipMemcpyPeerAsync(devs[g]->ytmp + off, devs[g]->dev, devs[0]->ytmp + off, devs[0]->dev, (size_t)count * sizeof(double), stream_of(streams, g)));
    HIPCHK(hipEventRecord(G->ev[n + g], stream_of(streams, g)));
  }
  HIPCHK(hipSetDevice(devs[0]->dev));
  for (int g = 1; g < n; g++) HIPCHK(hipStreamWaitEvent(stream_of(streams, 0), G->ev[n + g], 0)); // rank 0 goes on writing its vector
  return 0;
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

// the sweep templates that chol_api_schur.cpp calls (chol_device.h), for the two element types of the arena
template int form_inverses<double>(cholamd_device *, const double *, int, bool, hipStream_t);
template int sweep_levels<double>(cholamd_device *, const double *, sweep_rhs, bool, int, int, int64_t *, hipStream_t);
template int sweep_steps<double>(cholamd_device *, const double *, const sdet_dev &, int, sweep_rhs, int64_t *, hipStream_t);
template int form_inverses<float>(cholamd_device *, const float *, int, bool, hipStream_t);
template int sweep_levels<float>(cholamd_device *, const float *, sweep_rhs, bool, int, int, int64_t *, hipStream_t);
template int sweep_steps<float>(cholamd_device *, const float *, const sdet_dev &, int, sweep_rhs, int64_t *, hipStream_t);
