// Schur complement on the top k levels of the tree (cholamd_schur): S = A_TT - A_TI A_II^-1 A_IT, read out of the arena after the levels under the cut
// have been eliminated (cholamd_schur_factor), into a dense column-major m x m matrix with both triangles.
//
// A bandwidth kernel.  The list it is driven by (chol_schur_pieces with the empty pieces, cut into chunks of CHOL_SCHUR_CHUNK = 64 columns) tiles the LOWER
// triangle of S exactly once with pieces of at most 16 rows x 64 columns: one 16-row tile of a block of two kept separators -- 16 consecutive doubles per
// column of the panel, one 128-byte line -- or a piece without storage (off = -1: the two separators are not ancestor and descendant, or the row
// compaction dropped the tile), which is written as exact zeros.  One workgroup of 256 threads per piece:
//   read      lane = (row i = t & 15, column j = t >> 4 (+ 16 per pass)): a wave reads four whole 128-byte column segments of the panel
//   lower     S(row0 + i, col0 + j) with the same assignment: 128-byte segments of S's columns
//   upper     through LDS: the piece is parked as tile[j][i] (rows of 17 doubles: the writes of a 16-lane group and the reads of a 32-lane half each
//             touch every bank once), then lane = (column jj = t & 63, row ii = t >> 6 (+ 4 per pass)) writes S(col0 + jj, row0 + ii): a wave writes
//             64 consecutive doubles of one column of S instead of 64 strided ones
// A piece of a diagonal block means its lower triangle only (row0 + i >= col0 + j); its strict lower part is mirrored, the diagonal is written once.
// Every element of S therefore has exactly one owner: the lower triangle the piece that covers it, the upper triangle the mirror of the piece that covers
// its transpose.  No atomics, no read of S: two calls on one arena write the same bits.  Rows m .. lds - 1 of S are never addressed.
#include <hip/hip_runtime.h>

#include "chol_kernels.h"

#define SCH_W CHOL_SCHUR_CHUNK

__global__ __launch_bounds__(256) void k_schur_gather(const double *__restrict__ arena, const chol_schur_desc *__restrict__ descs, double *__restrict__ S, int64_t lds)
{
  __shared__ double tile[SCH_W][CHOL_NB + 1];
  const chol_schur_desc q = descs[blockIdx.x];
  {
    const int i = threadIdx.x & (CHOL_NB - 1), jq = threadIdx.x >> 4;
#pragma unroll
    for (int p = 0; p < SCH_W / 16; p++) {
      const int j = jq + 16 * p;
      const bool own = i < q.rows && j < q.cols && (!q.diag || q.row0 + i >= q.col0 + j);
      double v = 0.0;
      if (own && q.off >= 0) v = arena[q.off + i + (int64_t)j * q.ld];
      if (own) S[(int64_t)(q.row0 + i) + (int64_t)(q.col0 + j) * lds] = v;
      tile[j][i] = v;
    }
  }
  __syncthreads();
  {
    const int jj = threadIdx.x & (SCH_W - 1), iq = threadIdx.x >> 6;
#pragma unroll
    for (int p = 0; p < CHOL_NB / 4; p++) {
      const int ii = iq + 4 * p;
      if (ii < q.rows && jj < q.cols && (!q.diag || q.row0 + ii > q.col0 + jj))
        S[(int64_t)(q.col0 + jj) + (int64_t)(q.row0 + ii) * lds] = tile[jj][ii];
    }
  }
}

int chol_launch_schur_gather(const double *arena, const chol_schur_desc *descs, int64_t ndesc, double *S, int64_t lds, hipStream_t st)
{
  if (ndesc <= 0) return (int)hipSuccess;
  if (ndesc > 0x7fffffff) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_schur_gather, dim3((unsigned)ndesc), dim3(256), 0, st, arena, descs, S, lds);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Block forms of condense and expand (cholamd_schur_condense_nrhs / cholamd_schur_expand_nrhs): the transposing copies between the permuted ROW-major block
// of one chunk (Y: n x CHOL_NRHS_W, the 32 values of a permuted row are 256 contiguous bytes) and the caller's COLUMN-major arrays in permuted / Schur order.
// One workgroup of 256 threads per SNR_ROWS = 64 permuted rows, through an LDS tile [column][row] of pitch 65 doubles:
//   row-major side     element e = t + 256 p: row e / 32, column e % 32 -- a wave moves two whole rows of Y, 512 contiguous bytes; in LDS the 32 lanes of a
//                      half step the column (pitch 65 doubles, odd: 32 different bank pairs), the row is the half's own
//   column-major side  row t & 63, column (t >> 6) + 4 p -- a wave moves 64 consecutive doubles of ONE column of W / G / XT (512 contiguous bytes where the
//                      array is aligned), and 64 consecutive doubles of one LDS row
// No lane strides a leading dimension against its neighbour.  Rows >= n, rows of the tile past the array and columns >= cols are never addressed in the
// caller's arrays; the pack writes zeros into the block's padding columns (they stay zero through the sweeps).
// ---------------------------------------------------------------------------------------------
#define SNR_ROWS 64
#define SNR_PITCH (SNR_ROWS + 1)
static_assert(CHOL_NRHS_W == 32, "a half wave holds one row of the block");

// after the forward sweep: W(:, c0 + j) = Y(:, j) for all n rows (permuted order), G(i - t0, c0 + j) = Y(i, j) for the rows i >= t0
__global__ __launch_bounds__(256) void k_schur_unpack(const double *__restrict__ Y, int n, int t0, int c0, int cols, double *__restrict__ W, int64_t ldw,
                                                      double *__restrict__ G, int64_t ldg)
{
  __shared__ double tile[CHOL_NRHS_W][SNR_PITCH];
  const int r0 = blockIdx.x * SNR_ROWS;
#pragma unroll
  for (int p = 0; p < SNR_ROWS * CHOL_NRHS_W / 256; p++) {
    const int e = threadIdx.x + 256 * p, i = e / CHOL_NRHS_W, j = e % CHOL_NRHS_W;
    if (r0 + i < n) tile[j][i] = Y[(int64_t)(r0 + i) * CHOL_NRHS_W + j];
  }
  __syncthreads();
  const int i = threadIdx.x & (SNR_ROWS - 1), jq = threadIdx.x >> 6, r = r0 + i;
  if (r >= n) return;
#pragma unroll
  for (int p = 0; p < CHOL_NRHS_W / 4; p++) {
    const int j = jq + 4 * p;
    if (j >= cols) break;
    const double v = tile[j][i];
    W[(int64_t)r + (int64_t)(c0 + j) * ldw] = v;
    if (r >= t0) G[(int64_t)(r - t0) + (int64_t)(c0 + j) * ldg] = v;
  }
}
// before the backward sweep: Y(i, j) = W(i, c0 + j) for the rows i < t0, XT(i - t0, c0 + j) for the rows i >= t0, 0 for the padding columns j >= cols
__global__ __launch_bounds__(256) void k_schur_pack(const double *__restrict__ W, int64_t ldw, const double *__restrict__ XT, int64_t ldxt, int n, int t0, int c0,
                                                    int cols, double *__restrict__ Y)
{
  __shared__ double tile[CHOL_NRHS_W][SNR_PITCH];
  const int r0 = blockIdx.x * SNR_ROWS;
  {
    const int i = threadIdx.x & (SNR_ROWS - 1), jq = threadIdx.x >> 6, r = r0 + i;
#pragma unroll
    for (int p = 0; p < CHOL_NRHS_W / 4; p++) {
      const int j = jq + 4 * p;
      double v = 0.0;
      if (r < n && j < cols) v = r < t0 ? W[(int64_t)r + (int64_t)(c0 + j) * ldw] : XT[(int64_t)(r - t0) + (int64_t)(c0 + j) * ldxt];
      tile[j][i] = v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < SNR_ROWS * CHOL_NRHS_W / 256; p++) {
    const int e = threadIdx.x + 256 * p, i = e / CHOL_NRHS_W, j = e % CHOL_NRHS_W;
    if (r0 + i < n) Y[(int64_t)(r0 + i) * CHOL_NRHS_W + j] = tile[j][i];
  }
}
int chol_launch_schur_unpack(const double *Y, int n, int t0, int c0, int cols, double *W, int64_t ldw, double *G, int64_t ldg, hipStream_t st)
{
  if (n <= 0 || cols <= 0) return (int)hipSuccess;
  hipLaunchKernelGGL(k_schur_unpack, dim3((unsigned)((n + SNR_ROWS - 1) / SNR_ROWS)), dim3(256), 0, st, Y, n, t0, c0, cols, W, ldw, G, ldg);
  return (int)hipGetLastError();
}
int chol_launch_schur_pack(const double *W, int64_t ldw, const double *XT, int64_t ldxt, int n, int t0, int c0, int cols, double *Y, hipStream_t st)
{
  if (n <= 0 || cols <= 0) return (int)hipSuccess;
  hipLaunchKernelGGL(k_schur_pack, dim3((unsigned)((n + SNR_ROWS - 1) / SNR_ROWS)), dim3(256), 0, st, W, ldw, XT, ldxt, n, t0, c0, cols, Y);
  return (int)hipGetLastError();
}
