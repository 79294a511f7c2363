// C ABI glue of libcholamd, the factorisation: the one-launch program and the level loop of both precisions, the communicators (RCCL and local), the
// extend-add exchange, the broadcasts, the sharded and multi-rank factor and the gathers.  Compiled with hipcc like chol_api.cpp; what they share is in
// chol_device.h.
#include "chol_device.h"

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
int comm_matches(const cholamd_device *d, const cholamd_comm *c)
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

// one process driving n ranks: the two sums of the distributed solve (solve_multi_t in chol_api_solve.cpp; defined here, beside k_sum_ranks, so that one file
// instantiates the kernel) as an ordered device-side sum on rank 0's stream and peer copies back (local communicator), or grouped ncclAllReduce calls (cholamd_comm_create_all)
int multi_sum_vec(cholamd_device *const *devs, cholamd_comm *const *comms, int n, void *const *streams, int64_t off, int64_t count)
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
