// Internal header of the C ABI glue (chol_api*.cpp; never installed): the includes and error macros, the device and communicator objects and their
// parts, the scoped helpers of the sweeps and the timing, and the declarations of the helpers that one glue file defines and another one calls.
// Whatever a single file uses stays static in that file.
#ifndef CHOL_DEVICE_H
#define CHOL_DEVICE_H
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cfloat>
#include <cmath>
#include <cctype>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include <atomic>
#include "chol_devbuf.h"
#include "chol_kernels.h"
#include "chol_plan.h"
#include "cholamd.h"

#define HIPCHK(call)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess) {                                                                           \
      chol_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);     \
      return (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice) ? CHOLAMD_ERR_NO_DEVICE : CHOLAMD_ERR_HIP; \
    }                                                                                                 \
  } while (0)

#define NCCLCHK(call)                                                                                 \
  do {                                                                                                \
    ncclResult_t r_ = (call);                                                                         \
    if (r_ != ncclSuccess) {                                                                          \
      chol_set_error("%s failed: %s (%s:%d)", #call, ncclGetErrorString(r_), __FILE__, __LINE__);     \
      return CHOLAMD_ERR_COMM;                                                                        \
    }                                                                                                 \
  } while (0)

struct pinned_words { // pinned host memory, owned like a dev_buf: where status words are read back to
  int64_t *p = nullptr;
  pinned_words() = default; pinned_words(const pinned_words &) = delete; pinned_words &operator=(const pinned_words &) = delete;
  ~pinned_words() { if (p) (void)hipHostFree(p); }
  operator int64_t *() const { return p; }
  int ensure(size_t n) { if (!p) HIPCHK(hipHostMalloc((void **)&p, n * sizeof(int64_t))); return 0; }
};
struct sum_desc { int64_t off, count, stage; unsigned contrib, pad; };

struct level_dev {
  int n_potrf = 0, n_trsm = 0, n_task = 0, n_src = 0;
  std::vector<chol_phase> phase; // launches of the level in order (big pivots are factored in column blocks)
  dev_buf<chol_potrf_desc> potrf; dev_buf<chol_trsm_desc> trsm; // (potrf: with the role tables behind the descriptors, upload_level)
  dev_buf<chol_upd_task> task, task_mt; dev_buf<chol_upd_src> src;
  std::vector<chol_bcast> bcast;  // distributed top levels: the column blocks a phase of kind 6 broadcasts
};
struct solve_dev {
  int n_trsv = 0, n_grp = 0, n_fw = 0, n_bw = 0;
  dev_buf<chol_trsv_desc> trsv; dev_buf<chol_gemv_desc> fw, bw;
  dev_buf<int> grp_start, grp_rows, bw_start;
  int n_ifw = 0, n_ibw = 0, max_n = 0, max_under = 0;
  int64_t w256_off = -1; // this level's explicit span inverses in cholamd_device::w256 (levels of at most 8 separators wider than a span); -1: none
  dev_buf<int> ifw, ibw;
};
struct selinv_dev { // the lists of one tree level of the selected inversion (chol_selinv_level) on the device
  std::vector<chol_selinv_sep> host; // the separator descriptors, for the launch geometry of every step
  dev_buf<chol_selinv_sep> sep; dev_buf<chol_selinv_tile> tile;
  dev_buf<int> chain_ld, chain_pos0; dev_buf<int64_t> rowoff;
  int max_nblk = 0;
};
struct schur_dev { dev_buf<chol_schur_desc> desc; int64_t n = -1; }; // n < 0: not built yet
// deterministic step lists (chol_sdet_lists: the whole tree's, or those of condense / expand cut at k kept levels) on the device; the steps stay on the
// host: they are the launch sequence
struct sdet_dev { dev_buf<chol_mul_item> item[2]; dev_buf<chol_mul_src> src[2]; std::vector<chol_sdet_step> step[2]; bool ready = false; };
// kinds: 0 potrf (+ fused trsm), 1 trsm, 2 update, 3 program launch, 4 extend-add exchange (RCCL), 5 broadcasts of the distributed top levels
#define CHOL_TIMING_KINDS 8
#define CHOL_TK_EXCHANGE 4
#define CHOL_TK_BCAST 5
struct timed_launch { hipEvent_t a, b; int kind; };

struct cholamd_device {
  struct vmm_arena { void *va; size_t total; std::vector<hipMemGenericAllocationHandle_t> handles; };
  std::vector<vmm_arena> vmm; // sharded arenas of this rank (cholamd_device_alloc_arena)

  const cholamd_plan *plan = nullptr;
  int dev = 0, rank = 0, world = 1;
  std::vector<level_dev> lv;
  std::vector<solve_dev> sv;
  bool solve_ready = false;
  int solve_rank = 0, solve_world = 1; // the partition the solve lists were built for
  dev_buf<int> zr_sub; int n_zr_sub = 0; // distributed solve: (offset, length) ranges of the permuted vector this rank starts from zero in (other ranks' subtrees; the shared top on ranks other than 0)
  dev_buf<double> ws;
  dev_buf<double> ws_solve; // 16x16 inverses of the diagonal blocks of the arena being solved with
  dev_buf<int> step_flags;     // flags of the step launches of the wide top separators' span chains (k_solve_step): one per separator of a level, 64 ints
  int step_gen = 0;           // ... and the number of the last such launch (a flag equal to it: the launch's span is solved)
  dev_buf<double> w256;       // explicit inverses of the 256-column diagonal spans of the wide top separators (k_solve_inv256, recomputed with the 16x16 inverses)
  dev_buf<double> step_xt;    // 8 x 256 doubles: a step launch's x_k before it replaces the right-hand side
  bool keep_inverses = false; // the correction solves of a refinement: same factor as the solve before them, its diagonal inverses (16x16, spans) are kept
  dev_buf<int> info;        // [0] first failing column, [1] separator; two slots of two ints: the program launch alternates between them (each launch clears the other
                            // one for the next: no memset node per factorisation), every other path uses slot 0
  int *info_last = nullptr; // the slot of the most recent factorisation (cholamd_factor_info)
  int info_parity = 0; bool info_foreign = false; // program path: slot of the next launch; slot 0 was used by another path since
  dev_buf<int> progress;    // fused launches: columns published per pivot block (epoch * 64 + columns); [nsep + 1] = TRSM workgroups finished
  int epoch = 0, done_total = 0;
  dev_buf<int64_t> a_dst; dev_buf<double> a_val; dev_buf<int> perm; dev_buf<double> ytmp;
  // distributed top levels: the entries of A in the column blocks of the shared top THIS rank owns ([0]: by the fp64 schedule's blocks, [1]: the fp32 one's)
  // top_val is gathered on the device from a_val through top_e (the entries' positions in the scatter list), so that it follows cholamd_device_set_values
  dev_buf<int64_t> top_dst[2]; dev_buf<double> top_val[2]; dev_buf<int> top_e[2]; int64_t top_n[2] = { 0, 0 }; int top_gen[2] = { -1, -1 };
  // new values of A (cholamd_device_set_values): the index lists of the gather and the entries' classes (uploaded at the first call), the status words of
  // the last call on the device ([4]), their start values ([4], device) and where they are read back to (pinned host, two slots of four)
  dev_buf<int> a_src, csr_src; dev_buf<unsigned char> e_cls;
  dev_buf<int> e_row, e_col; // the entry list itself (cholamd_values_grad_pairs / _logdet: uploaded at the first call)
  dev_buf<int64_t> vs_dev, vs_init; pinned_words vs_host;
  int64_t vs_last[4] = { 0, 0, 0, 0 };  // the last call's status words as read back
  bool vs_called = false, vs_last_valid = false;
  bool vs_in_force = false; // the values in force come from set_values: the fp32 range verdict comes from the status words, not from the plan's values
  bool f32_pending = false; // ... and has not been read back yet (the last call was asynchronous)
  bool timing = false;
  std::vector<timed_launch> tl;
  std::vector<hipEvent_t> pool;
  // the one-launch program of the whole factorisation (single GPU, small problems: chol_build_program / k_program)
  level_dev prog;
  dev_buf<chol_job> jobs; dev_buf<chol_wait> pwaits; dev_buf<chol_ext> exts;
  dev_buf<int> pctr, pctr_total; // counters (last one: the queue head) and what one factorisation adds to each
  int n_job = 0, n_pctr = 0, prog_grid = 0, prog_epoch = 0, prog_epoch_limit = 0;
  bool prog_ready = false;
  unsigned long long *trace = nullptr; // diagnostic: per-job clock stamps of the next program launches (cholamd_device_program_trace, which owns them)
  std::vector<chol_job> jobs_host;
  // mixed precision (fp32 factor + fp64 refinement): work lists of the fp32 kernels, their workspace, A as a device CSR
  std::vector<level_dev> lv32;
  dev_buf<float> ws32;
  int f32_range = -1; int64_t f32_bad = -1; // A's entries all zero or normal floats (1), or not (0: f32_bad = the first entry that is not); -1: not checked yet
  dev_buf<int64_t> csr_ptr; dev_buf<int> csr_col; dev_buf<double> csr_val;
  dev_buf<double> rvec, dxvec, partial;
  // extend-add exchange under the distributed top levels: staging of the copies received for the owned column blocks, descriptors of the sum
  dev_buf<char> xstage; size_t xstage_bytes = 0; dev_buf<sum_desc> xdesc; int xdesc_gen = -1, xdesc_elem = 0, sched_gen = 0;
  // switches, read from the environment once at cholamd_device_create (cholamd_device_set_option changes them later)
  chol_sched_opts opt;
  bool solve_reference_shape = false; // cholamd_solve with the per-call (deterministic) kernels of the BLAS-level entry points
  // option solve_deterministic: the streamed sweeps with owner gathers in place of the atomic kernels (chol_solve_det.hip).  The step lists of both
  // directions (chol_sdet_lists) are built and uploaded at the first such solve
  bool solve_deterministic = false;
  // option solve_deterministic_block: under solve_deterministic (and without solve_reference_shape) the _nrhs entry points take the deterministic BLOCK path
  // (solve_nrhs_t with the same step lists on chunks of 32 columns) instead of going column by column; no effect otherwise
  bool solve_deterministic_block = false;
  sdet_dev sdet;
  // block solve (cholamd_solve_nrhs): the permuted block of one chunk (n x CHOL_NRHS_W, row-major); refinement: the chunk's right-hand sides, residual and
  // correction (n x CHOL_NRHS_W, column-major) and the per-column partial sums of the residual kernel
  dev_buf<double> ynrhs, bnrhs, rnrhs, dxnrhs, pnrhs;
  // factor queries (cholamd_factor_diag / _logdet): the TRSV descriptors of the whole tree in one list ordered by permuted position and the prefix of their
  // column counts (built with the solve lists of rank 0 of 1); the logdet's per-workgroup partial sums, their integer companions and the three result words
  dev_buf<chol_trsv_desc> dg_desc; dev_buf<int> dg_prefix; int n_dg = 0;
  dev_buf<double> ld_part; dev_buf<int64_t> ld_ipart, ld_res;
  // selected inversion (cholamd_selinv): the gather lists of every level and the workspace of the widest level, built at the first call
  std::vector<selinv_dev> si; dev_buf<double> si_ws; bool si_ready = false;
  // Schur complement (cholamd_schur): the gather kernel's piece list per number of kept levels k (index k), uploaded at the first call with that k
  std::vector<schur_dev> sc;
  // option schur_deterministic: condense / expand (single vector and _nrhs) walk the step lists cut at k (index k), built and uploaded at the first such
  // call with that k.  schur_launches: { atomic sweep, deterministic gather, deterministic span, pack / unpack } launches of the Schur sweeps so far
  bool schur_deterministic = false;
  std::vector<sdet_dev> scd;
  int64_t schur_launches[4] = { 0, 0, 0, 0 };
  // forward products (cholamd_multiply_half / cholamd_multiply / cholamd_factor_residual): the owner lists of the whole tree per direction, uploaded at the
  // first call; the intermediate vector of cholamd_multiply (permuted coordinates); the residual's per-workgroup partial sums and result words
  dev_buf<chol_mul_item> mul_item[2]; dev_buf<chol_mul_src> mul_src[2]; int n_mul_item[2] = { 0, 0 }; bool mul_ready = false;
  dev_buf<double> mvec, mr_part; dev_buf<int64_t> mr_ipart, mr_res;
  // their block form (cholamd_multiply_half_nrhs / cholamd_multiply_nrhs): the two permuted blocks of one chunk (n x CHOL_NRHS_W, row-major), allocated at the
  // first chunk that takes the block kernel; option multiply_nrhs_min: chunks of fewer columns go column by column (<= 0: the measured default)
  dev_buf<double> mznrhs, mwnrhs;
  int multiply_nrhs_min = 0;
  // preconditioned conjugate gradients (cholamd_solve_pcg*): the chunk's right-hand sides, p, q, r, z (n x CHOL_NRHS_W, column-major), one partial per
  // (column, workgroup), the columns' scalar records and where they are read back to; allocated at the first call
  dev_buf<double> pcg_b, pcg_p, pcg_q, pcg_r, pcg_z, pcg_part;
  dev_buf<chol_pcg_rec> pcg_rec; pinned_words pcg_host;
};

// A LOCAL communicator (cholamd_comm_create_local) joins rank objects of ONE process without RCCL: the exchange is a device-side
// ordered sum of the tails and peer copies, events order the ranks' streams.  The ranks may share a device (how the one-GPU test
// box runs world 2 ... 8); usable through cholamd_factor_multi only, which sees every rank's arena.
struct local_group {
  int n = 0, refs = 0;
  std::vector<int> dev;
  std::vector<hipEvent_t> ev; // [g]: rank g's stream has reached the exchange; [n + g]: rank g's part of the exchange is enqueued
};
struct cholamd_comm {
  ncclComm_t comm = nullptr;
  int world = 1, rank = 0;
  bool owned = true;
  local_group *local = nullptr;
};

struct keep_inverses_scope { // set on the devices of a refinement after its first solve, cleared on every way out
  cholamd_device *const *devs; int n;
  keep_inverses_scope(cholamd_device *const *devs_, int n_) : devs(devs_), n(n_) { for (int g = 0; g < n; g++) devs[g]->keep_inverses = true; }
  ~keep_inverses_scope() { for (int g = 0; g < n; g++) devs[g]->keep_inverses = false; }
};
// which sweeps a body runs: one CHOLAMD_HALF_* sweep alone, or FORWARD then BACKWARD (the products: BACKWARD then FORWARD)
#define CHOL_BOTH_SWEEPS (-1)
// what a sweep works on: the permuted vector (n doubles), or the permuted row-major block of one chunk (n x CHOL_NRHS_W) with the chol_nrhs_* kernels
struct sweep_rhs { double *y; bool block; };
struct keep_restore { // keep_inverses for the chunks of one call, the caller's value back on every way out
  cholamd_device *d; bool old;
  explicit keep_restore(cholamd_device *d_) : d(d_), old(d_->keep_inverses) {}
  ~keep_restore() { d->keep_inverses = old; }
};
// The same rule for one triangular half (cholamd_solve_half_nrhs): a half chunk and a half single solve both drop one of the two sweeps.  DESIGN.md section 10
// records the measurement behind the value.
template <class TL> static constexpr int half_nrhs_min_block() { return sizeof(TL) == sizeof(double) ? 4 : 6; }

#pragma GCC visibility push(hidden) // helpers that cross glue files, by the file that defines them: none of them enters the library's dynamic symbol table
// chol_api.cpp
hipEvent_t get_event(cholamd_device *d);
int no_device_error();
bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb);
void free_solve_lists(cholamd_device *d);
int upload_level(level_dev &l, const chol_level_work &w, bool with_tables = true);
int clear_owned(cholamd_device *d, void *arena, size_t elem, hipStream_t st);
int f32_range_ok(cholamd_device *d, hipStream_t st);
int ensure_csr(cholamd_device *d);
int ensure_refine(cholamd_device *d);
// chol_api_factor.cpp
int comm_matches(const cholamd_device *d, const cholamd_comm *c);
int multi_sum_vec(cholamd_device *const *devs, cholamd_comm *const *comms, int n, void *const *streams, int64_t off, int64_t count);
// chol_api_solve.cpp
int build_solve(cholamd_device *d, int rank = 0, int world = 1);
int upload_sdet(sdet_dev &q, const chol_sdet_lists &w);
hipStream_t stream_of(void *const *streams, int g);
int half_which_ok(int which, const char *what);
int block_check(cholamd_device *d, bool with_arena, const void *arena, const double *B, int64_t ldb, const double *X, int64_t ldx, int nrhs, const char *what, const char *in,
                const char *out);
int nrhs_check(cholamd_device *d, const void *arena, const double *B, int64_t ldb, const double *X, int64_t ldx, int nrhs, const char *what, const char *in = "B", const char *out = "X");
// (the templates: instantiated in chol_api_solve.cpp for double and float)
template <class TL> int form_inverses(cholamd_device *d, const TL *d_arena, int lvl_lo, bool with_spans, hipStream_t st);
template <class TL> int sweep_levels(cholamd_device *d, const TL *d_arena, sweep_rhs rhs, bool backward, int lvl_lo, int lvl_hi, int64_t *count, hipStream_t st);
template <class TL> int sweep_steps(cholamd_device *d, const TL *d_arena, const sdet_dev &c, int q, sweep_rhs rhs, int64_t *counts, hipStream_t st);
template <class TL> int solve_any(cholamd_device *d, const TL *d_arena, const double *d_b, double *d_x, int which, hipStream_t st);
template <class TL> int solve_nrhs_any(cholamd_device *d, const TL *d_arena, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int cols, bool half, int which, hipStream_t st);
#pragma GCC visibility pop

struct scoped_timer {
  cholamd_device *d; hipStream_t st; int kind; hipEvent_t a{}, b{}; bool on;
  scoped_timer(cholamd_device *d_, hipStream_t st_, int kind_, bool active) : d(d_), st(st_), kind(kind_), on(d_->timing && active)
  {
    if (on) { a = get_event(d); b = get_event(d); (void)hipEventRecord(a, st); }
  }
  ~scoped_timer()
  {
    if (on) { (void)hipEventRecord(b, st); d->tl.push_back({ a, b, kind }); }
  }
};
#endif
