// Sparse solves (cholamd_sparse_*; include/cholamd.h at "sparse solves"): the two kernels around the pruned sweeps.  The sweeps
// themselves are the block kernels of the deterministic solve (k_solve_det_gather_nrhs, k_nrhs_span, k_solve_dinv) on the pruned lists; what is new is how
// a chunk of CHOL_NRHS_W = 32 columns gets into and out of the permuted row-major block Y (n x 32) WITHOUT touching its inactive rows: at 100^3 the block is
// 256 MB, and clearing it whole would cost more than the pruned sweeps.
//   load   one launch over the ACTIVE rows (act_pos: the positions of up(in) | up(out), ascending).  Row r of the list is either the row of input dof
//          act_in[r] -- Y[act_pos[r] 32 + j] = Bs[act_in[r] + (c0 + j) ldb] for j < cols, 0.0 for the padding columns of a short chunk -- or (act_in[r] < 0)
//          a row that starts from zero: the forward sweep's fill-in, and the rows of up(out) outside up(in), which the backward sweep reads as the forward
//          results they structurally are.  All 32 columns of every active row are written, so nothing an earlier call left in them survives.
//   store  Xs[i + (c0 + j) ldx] = Y[pos_out[i] 32 + j] for j < cols.
// One owner per element, no atomics, plain vector stores.  A row of Y is a 256-byte line: 32 consecutive lanes write (load) or read (store) one line.  The
// caller's blocks are column-major, so their side of the copy is strided; it is n_in + n_out rows in all.
#include <hip/hip_runtime.h>

#include "chol_kernels.h"

#define SPW CHOL_NRHS_W
static_assert(SPW == 32, "a row of the block is 32 doubles: half a wave per line");

__global__ __launch_bounds__(256) void k_sparse_load(const double *__restrict__ Bs, int64_t ldb, const int *__restrict__ act_pos, const int *__restrict__ act_in, int64_t n_pos,
                                                     int c0, int cols, double *__restrict__ Y)
{
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_pos * SPW) return;
  const int64_t r = e / SPW;
  const int j = (int)(e % SPW), i = act_in[r];
  Y[(int64_t)act_pos[r] * SPW + j] = i >= 0 && j < cols ? Bs[i + (int64_t)(c0 + j) * ldb] : 0.0;
}
__global__ __launch_bounds__(256) void k_sparse_store(const double *__restrict__ Y, const int *__restrict__ pos_out, int64_t n_out, double *__restrict__ Xs, int64_t ldx, int c0, int cols)
{
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_out * SPW) return;
  const int64_t i = e / SPW;
  const int j = (int)(e % SPW);
  if (j < cols) Xs[i + (int64_t)(c0 + j) * ldx] = Y[(int64_t)pos_out[i] * SPW + j];
}

int chol_launch_sparse_load(const double *Bs, int64_t ldb, const int *act_pos, const int *act_in, int64_t n_pos, int c0, int cols, double *Y, hipStream_t st)
{
  if (n_pos <= 0) return 0;
  hipLaunchKernelGGL(k_sparse_load, dim3((unsigned)((n_pos * SPW + 255) / 256)), dim3(256), 0, st, Bs, ldb, act_pos, act_in, n_pos, c0, cols, Y);
  return (int)hipGetLastError();
}
int chol_launch_sparse_store(const double *Y, const int *pos_out, int64_t n_out, double *Xs, int64_t ldx, int c0, int cols, hipStream_t st)
{
  if (n_out <= 0) return 0;
  hipLaunchKernelGGL(k_sparse_store, dim3((unsigned)((n_out * SPW + 255) / 256)), dim3(256), 0, st, Y, pos_out, n_out, Xs, ldx, c0, cols);
  return (int)hipGetLastError();
}
