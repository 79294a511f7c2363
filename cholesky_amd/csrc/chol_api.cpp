// C ABI glue of libcholamd: the device object (its work lists, buffers, rank arenas and timing) and the values of A on it.  Every other family of entry
// points has a chol_api_*.cpp file of its own over chol_device.h.  Compiled with hipcc; everything exported is extern "C" (include/cholamd.h).
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

void free_solve_lists(cholamd_device *d)
{
  d->sv.clear(); d->solve_ready = false;
  d->w256.reset(); d->dg_desc.reset(); d->dg_prefix.reset(); d->zr_sub.reset(); d->n_dg = 0; d->n_zr_sub = 0;
}
int upload_level(level_dev &l, const chol_level_work &w, bool with_tables)
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
int clear_owned(cholamd_device *d, void *arena, size_t elem, hipStream_t st)
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
int f32_range_ok(cholamd_device *d, hipStream_t st)
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
int ensure_csr(cholamd_device *d)
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
int ensure_refine(cholamd_device *d)
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
