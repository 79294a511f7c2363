// The gathers of the deterministic streamed solve (option solve_deterministic; include/cholamd.h at "deterministic solve", lists: chol_plan.h at
// chol_sdet_lists).  A sweep is a chain of STEPS, level by level: a level's lead step subtracts from the level's part of the permuted vector what reaches
// it from outside its own diagonal blocks (FORWARD: the panels of the descendants; BACKWARD: the row runs into the ancestors); then, per 256-column span of
// the level's separators, a step subtracts what reaches the span from inside the block and the span solvers of chol_kernels.hip (chol_launch_solve_span,
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
