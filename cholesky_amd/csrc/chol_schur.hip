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
