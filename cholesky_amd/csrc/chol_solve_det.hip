// The gathers of the deterministic streamed solve (option solve_deterministic; include/cholamd.h at "deterministic solve", lists: chol_plan.h at
// chol_sdet_lists).  A sweep is a chain of STEPS, level by level: a level's lead step subtracts from the level's part of the permuted vector what reaches
// it from outside its own diagonal blocks (FORWARD: the panels of the descendants; BACKWARD: the row runs into the ancestors); then, per 256-column span of
// the level's separators, a step subtracts what reaches the span from inside the block and the span solvers of chol_solve.hip (chol_launch_solve_span,
// plain stores) solve the span.  This kernel is the gather of either kind of step.  One workgroup per ITEM, an item owns at most 16 consecutive positions
// and walks its sources in list order: one owner per position, a fixed summation order, no floating-point atomics -- two sweeps over one arena and one
// right-hand side leave the same bits.  What a step reads of the vector was written by earlier launches on the stream (descendants and earlier spans in the
// FORWARD sweep, ancestors and later spans in the BACKWARD one) and is owned by no item of the step, so a launch has no order among its workgroups to
// respect: no waiting, no flags.
//
// Shape: k_multiply's (chol_multiply.hip).  The 256 lanes form a 16 x 16 grid, `in` = lane & 15 along a column of the column-major panel (stride 1), `out` =
// lane >> 4 across 16 columns (stride ld); every group of 16 lanes reads one whole 128-byte segment per step (64 bytes of an fp32 factor).
//   FORWARD   the item owns 16 ROWS: in = the row, out = the column modulo 16; a lane sums its row over the columns out, out + 16, ...
//   BACKWARD  the item owns 16 COLUMNS: out = the column, in = the row modulo 16; a lane sums its column over the rows in, in + 16, ...
// The reduction index advances in blocks of 256 steps whose vector values are staged in LDS by one coalesced load; the 16 loads of a block are issued back
// to back before the first multiply.  The 16 partial sums of every owned line are added in a fixed order out of LDS and subtracted from the owner's value.
// Lines beyond the item's nv and steps beyond a source's length are never loaded.  Every source of these lists is meant whole (the triangles are the span
// solvers' business), so there is no triangle rule here.  The factor's element type is a template parameter; everything after the load is fp64.
#include <hip/hip_runtime.h>

#include "chol_kernels.h"
#include "chol_plan.h"

#define SDET_THREADS 256
#define SDET_STEPS (SDET_THREADS / CHOL_MUL_TILE) // reduction steps a lane takes per staged block of the vector
#define SDET_RED_LD (CHOL_MUL_TILE + 1)

template <class TL, int BW>
__global__ __launch_bounds__(SDET_THREADS) void k_solve_det_gather(const TL *__restrict__ base, const chol_mul_item *__restrict__ items, const chol_mul_src *__restrict__ srcs, double *y)
{
  __shared__ double zs[SDET_THREADS];
  __shared__ double red[CHOL_MUL_TILE * SDET_RED_LD]; // rows padded to 17: lanes that are 16 entries apart would share a bank
  const chol_mul_item it = items[blockIdx.x];
  const int t = threadIdx.x, in = t & (CHOL_MUL_TILE - 1), out = t >> 4;
  const int line = BW ? out : in;   // the owned line of this lane
  const int red0 = BW ? in : out;   // its place among the 16 lanes that share the line
  const bool owns = line < it.nv;
  double acc = 0.0;
  for (int s = it.src_first; s < it.src_end; s++) {
    const chol_mul_src q = srcs[s];
    const TL *__restrict__ a = base + q.a_off + (BW ? (int64_t)line * q.ld : (int64_t)line);
    for (int kb = 0; kb < q.len; kb += SDET_THREADS) {
      __syncthreads(); // the previous block's zs are read
      zs[t] = kb + t < q.len ? y[q.z_off + kb + t] : 0.0;
      __syncthreads();
      double v[SDET_STEPS];
      bool ok[SDET_STEPS];
#pragma unroll
      for (int j = 0; j < SDET_STEPS; j++) {
        const int k = kb + j * CHOL_MUL_TILE + red0;
        ok[j] = owns && k < q.len;
        v[j] = ok[j] ? (double)a[BW ? (int64_t)k : (int64_t)k * q.ld] : 0.0;
      }
#pragma unroll
      for (int j = 0; j < SDET_STEPS; j++)
        if (ok[j]) acc = fma(v[j], zs[j * CHOL_MUL_TILE + red0], acc);
    }
  }
  __syncthreads();
  red[line * SDET_RED_LD + red0] = acc;
  __syncthreads();
  if (t < it.nv) {
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < CHOL_MUL_TILE; j++) sum += red[t * SDET_RED_LD + j];
    y[it.y_off + t] -= sum;
  }
}

template <class TL>
int chol_launch_solve_det_gather(const TL *base, const chol_mul_item *items, int n_items, const chol_mul_src *srcs, int backward, double *y, hipStream_t st)
{
  if (n_items <= 0) return 0;
  if (backward) hipLaunchKernelGGL((k_solve_det_gather<TL, 1>), dim3(n_items), dim3(SDET_THREADS), 0, st, base, items, srcs, y);
  else hipLaunchKernelGGL((k_solve_det_gather<TL, 0>), dim3(n_items), dim3(SDET_THREADS), 0, st, base, items, srcs, y);
  return (int)hipGetLastError();
}

template int chol_launch_solve_det_gather(const double *, const chol_mul_item *, int, const chol_mul_src *, int, double *, hipStream_t);
template int chol_launch_solve_det_gather(const float *, const chol_mul_item *, int, const chol_mul_src *, int, double *, hipStream_t);

// Block form (option solve_deterministic_block): the gather of a step on a chunk of CHOL_NRHS_W = 32 columns, Yp[(y_off + line) 32 + j] -= sum over the
// item's sources of L(line, k) Yp[(z_off + k) 32 + j].  Yp is the permuted ROW-major block of the block solve (k_nrhs_permute_in, padding columns zero).
// It is k_multiply_nrhs (chol_multiply_nrhs.hip) turned into a subtracting gather: one workgroup of CHOL_MULN_WAVES = 4 waves per item, every source's
// reduction range cut into chunks of CHOL_MULN_KSTEP steps dealt to the waves by chol_muln_wave, operands and their clamping from chol_muln_elem (an operand
// that is not meant is SELECTED to 0.0, never multiplied; the lists' `tri` values make every source whole), one 16 x 32 partial tile per wave in two
// v_mfma_f64_16x16x4_f64 accumulators, the four tiles added in wave order out of LDS by the element's owner.  One owner per element, a fixed order, no
// floating-point atomics, no waiting: two calls leave the same bits, and a column's bits depend on that column alone (an MFMA result column reads one column
// of B; padding columns and other columns never mix in).
//
// IN PLACE: the B operand and the result are the same buffer, so Yp carries no __restrict__.  That is safe because the rows a step READS (z_off + k) were
// solved by earlier launches on the stream and are owned by no item of the step (chol_build_solve_det checks both), and the rows an item WRITES are its own
// alone, read (for the subtraction) by their owner only: no workgroup of a launch reads what another one writes.
//
// Reduction tiles in LDS: pitch 32 doubles, not padded.  The stores are ds_write_b64 (lane groups of 16 contiguous lanes, bank = dword mod 32): a group
// is one lane group g of the MFMA result, 16 consecutive doubles of one row = 32 distinct banks at any pitch.  The reads are ds_read_b64 (two groups of 32
// lanes, bank = dword mod 64): 32 consecutive lanes read the 32 consecutive doubles of one row = 64 distinct banks.  (k_multiply_nrhs pads to 33 for its
// other read order, along the lines of one column; this kernel has the row order only.)
#define SDN_THREADS (64 * CHOL_MULN_WAVES)
#define SDN_U (CHOL_MULN_KSTEP / 4) // MFMA steps per chunk
#define SDN_NW CHOL_NRHS_W
#define SDN_TILE (CHOL_MUL_TILE * SDN_NW)
static_assert(SDN_NW == 32 && CHOL_MUL_TILE == 16 && CHOL_MULN_WAVES == 4, "a tile is 16 lines x two 16-column halves, four waves per item");

typedef double sdn_d4 __attribute__((ext_vector_type(4)));

template <class TL, int BW>
__global__ __launch_bounds__(SDN_THREADS) void k_solve_det_gather_nrhs(const TL *__restrict__ base, const chol_mul_item *__restrict__ items, const chol_mul_src *__restrict__ srcs, double *Yp)
{
  __shared__ double red[CHOL_MULN_WAVES * SDN_TILE];
  const chol_mul_item it = items[blockIdx.x];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i16 = lane & 15, g = lane >> 4;
  sdn_d4 acc0 = { 0.0, 0.0, 0.0, 0.0 }, acc1 = { 0.0, 0.0, 0.0, 0.0 };
  for (int s = it.src_first; s < it.src_end; s++) {
    const chol_mul_src q = srcs[s];
    const double *B = Yp + (int64_t)q.z_off * SDN_NW;
    // this wave's chunks of the source: c = first, first + 4, ... with chol_muln_wave(s - src_first, c) == wave
    const int first = (wave - (s - it.src_first)) & (CHOL_MULN_WAVES - 1);
    for (int k0 = first * CHOL_MULN_KSTEP; k0 < q.len; k0 += CHOL_MULN_WAVES * CHOL_MULN_KSTEP) {
      double a[SDN_U], b0[SDN_U], b1[SDN_U];
#pragma unroll
      for (int u = 0; u < SDN_U; ++u) {
        const int k = k0 + 4 * u + g, kk = min(k, q.len - 1);
        int meant;
        const int64_t e = chol_muln_elem(&q, BW, it.nv, i16, k, &meant);
        const double v = (double)base[e];
        a[u] = meant ? v : 0.0;
        const double z0 = B[(int64_t)kk * SDN_NW + i16], z1 = B[(int64_t)kk * SDN_NW + 16 + i16];
        b0[u] = k < q.len ? z0 : 0.0;
        b1[u] = k < q.len ? z1 : 0.0;
      }
#pragma unroll
      for (int u = 0; u < SDN_U; ++u) {
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b0[u], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b1[u], acc1, 0, 0, 0);
      }
    }
  }
  double *mine = red + wave * SDN_TILE;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mine[(g + 4 * r) * SDN_NW + i16] = acc0[r];
    mine[(g + 4 * r) * SDN_NW + 16 + i16] = acc1[r];
  }
  __syncthreads();
  // 512 elements, two per lane along the 32 columns of a row of the block, the waves' partial tiles in wave order
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int e = t + h * SDN_THREADS, line = e / SDN_NW;
    double sum = red[e];
#pragma unroll
    for (int w = 1; w < CHOL_MULN_WAVES; ++w) sum += red[w * SDN_TILE + e];
    if (line < it.nv) Yp[(int64_t)it.y_off * SDN_NW + e] -= sum;
  }
}

template <class TL>
int chol_launch_solve_det_gather_nrhs(const TL *base, const chol_mul_item *items, int n_items, const chol_mul_src *srcs, int backward, double *Yp, hipStream_t st)
{
  if (n_items <= 0) return 0;
  if (backward) hipLaunchKernelGGL((k_solve_det_gather_nrhs<TL, 1>), dim3(n_items), dim3(SDN_THREADS), 0, st, base, items, srcs, Yp);
  else hipLaunchKernelGGL((k_solve_det_gather_nrhs<TL, 0>), dim3(n_items), dim3(SDN_THREADS), 0, st, base, items, srcs, Yp);
  return (int)hipGetLastError();
}

template int chol_launch_solve_det_gather_nrhs(const double *, const chol_mul_item *, int, const chol_mul_src *, int, double *, hipStream_t);
template int chol_launch_solve_det_gather_nrhs(const float *, const chol_mul_item *, int, const chol_mul_src *, int, double *, hipStream_t);
