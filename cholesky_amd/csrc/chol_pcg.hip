// Preconditioned conjugate gradients with the factor in the arena as M (include/cholamd.h at cholamd_solve_pcg): the vector kernels of the loop and the
// operator y = A x of cholamd_apply.  Everything is fp64; vectors are in original dof order, blocks column-major n x cols with a leading dimension, every
// index is row + (int64) column * ld.  The layout is that of k_residual_csr / k_nrhs_residual: 256 rows per workgroup, one lane per row, columns on grid.y
// (the apply kernel: groups of G columns on grid.y, G accumulators per lane, so that a chunk reads the CSR cols / G times and not cols times).
//
// Every output element has one owner and is written with a plain store; there are no atomics, flags, spin-waits or cooperative launches: the kernel
// boundaries on the stream are the only ordering.  Nothing is read at a row >= n; the lanes of a ragged last workgroup contribute exact zeros to a partial
// by selection.  A partial is the workgroup's sum in the order of k_residual_csr: the shuffle tree of each wave, then ((w0 + w1) + w2) + w3; it does not
// depend on which other columns are in the launch, so a column of a block has the bits of the single-vector call.
//
// The scalars of the iteration live in one chol_pcg_rec per column in device memory.  k_pcg_scalars (one workgroup per column) adds the column's partials
// in ascending workgroup order and moves the record on; the vector kernels read alpha / beta from it.  A column whose state is not RUNNING gets
// alpha = beta = 0 and the vector kernels then SELECT (no multiplication by zero): its x and r are not written, its p becomes z.  Such a column never
// forms 0 / 0, and a NaN in it stays in it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "chol_kernels.h"

namespace {
// one workgroup's sum of v over its 256 lanes, in the order of k_residual_csr; valid in thread 0.  s: 4 doubles of LDS
__device__ __forceinline__ double wg_sum(double v, double *s)
{
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s[0] + s[1]) + s[2]) + s[3];
}

// apply: Q(:, j) = A P(:, j) for the columns j0 + g, g < G, of this workgroup's column group; acc = fma(val[e], p[col[e]], acc) with e ascending from 0.0
// (the order of cholamd_plan_apply_host).  partial != NULL: partial[j * gridDim.x + workgroup] = the workgroup's sum of p_i q_i.
template <int G>
__global__ __launch_bounds__(256) void k_pcg_apply(const int64_t *__restrict__ ptr, const int *__restrict__ col, const double *__restrict__ val,
                                                   const double *__restrict__ P, int64_t ldp, double *__restrict__ Q, int64_t ldq, int n, int cols,
                                                   double *__restrict__ partial)
{
  __shared__ double s[G][4];
  const int i = blockIdx.x * 256 + threadIdx.x, j0 = blockIdx.y * G;
  const int ng = min(G, cols - j0);
  double acc[G], pq[G];
#pragma unroll
  for (int g = 0; g < G; g++) { acc[g] = 0.0; pq[g] = 0.0; }
  if (i < n) {
    const double *p0 = P + (int64_t)j0 * ldp;
    for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
      const double v = val[e];
      const double *pc = p0 + col[e];
#pragma unroll
      for (int g = 0; g < G; g++)
        if (g < ng) acc[g] = fma(v, pc[(int64_t)g * ldp], acc[g]);
    }
#pragma unroll
    for (int g = 0; g < G; g++)
      if (g < ng) {
        Q[i + (int64_t)(j0 + g) * ldq] = acc[g];
        if (partial) pq[g] = p0[i + (int64_t)g * ldp] * acc[g];
      }
  }
  if (!partial) return;
#pragma unroll
  for (int g = 0; g < G; g++) {
    double a = pq[g];
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
    if ((threadIdx.x & 63) == 0) s[g][threadIdx.x >> 6] = a;
  }
  __syncthreads();
  if (threadIdx.x < ng) {
    const int g = threadIdx.x;
    partial[(int64_t)(j0 + g) * gridDim.x + blockIdx.x] = ((s[g][0] + s[g][1]) + s[g][2]) + s[g][3];
  }
}

// update: x += alpha_j p, r -= alpha_j q (alpha_j == 0: neither is written), partial of r_i^2; grid (row blocks, columns)
__global__ __launch_bounds__(256) void k_pcg_update(const chol_pcg_rec *__restrict__ rec, const double *__restrict__ P, const double *__restrict__ Q,
                                                    double *__restrict__ X, int64_t ldx, double *__restrict__ R, int64_t ld, int n, double *__restrict__ partial)
{
  __shared__ double s[4];
  const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  const double alpha = rec[j].alpha;
  double ri = 0.0;
  if (i < n) {
    const int64_t k = i + (int64_t)j * ld, kx = i + (int64_t)j * ldx;
    ri = R[k];
    if (alpha != 0.0) {
      X[kx] = fma(alpha, P[k], X[kx]);
      ri = fma(-alpha, Q[k], ri);
      R[k] = ri;
    }
  }
  const double t = wg_sum(ri * ri, s);
  if (threadIdx.x == 0) partial[(int64_t)j * gridDim.x + blockIdx.x] = t;
}
// dot: partial of r_i z_i
__global__ __launch_bounds__(256) void k_pcg_dot(const double *__restrict__ R, const double *__restrict__ Z, int64_t ld, int n, double *__restrict__ partial)
{
  __shared__ double s[4];
  const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  double v = 0.0;
  if (i < n) { const int64_t k = i + (int64_t)j * ld; v = R[k] * Z[k]; }
  const double t = wg_sum(v, s);
  if (threadIdx.x == 0) partial[(int64_t)j * gridDim.x + blockIdx.x] = t;
}
// direction: p = z + beta_j p (beta_j == 0: p = z, p is not read)
__global__ __launch_bounds__(256) void k_pcg_direction(const chol_pcg_rec *__restrict__ rec, const double *__restrict__ Z, double *__restrict__ P, int64_t ld, int n)
{
  const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  if (i >= n) return;
  const double beta = rec[j].beta;
  const int64_t k = i + (int64_t)j * ld;
  const double z = Z[k];
  P[k] = beta != 0.0 ? fma(beta, P[k], z) : z;
}
// take: r = t for the columns whose claim of convergence the true residual t did not bear out (state RESTART)
__global__ __launch_bounds__(256) void k_pcg_take(const chol_pcg_rec *__restrict__ rec, const double *__restrict__ T, double *__restrict__ R, int64_t ld, int n)
{
  const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  if (i >= n || rec[j].state != CHOL_PCG_RESTART) return;
  const int64_t k = i + (int64_t)j * ld;
  R[k] = T[k];
}

__device__ __forceinline__ bool pcg_finite(double v) { return v - v == 0.0; }
// scalars: one workgroup per column.  The column's nb partials (stride `stride` doubles from partial + j * nb * stride; the second quantity of the residual
// kernels' pairs at + 1) are staged through LDS 256 at a time and added by thread 0 in ascending workgroup order; `stage` says which scalar they are.
__global__ __launch_bounds__(256) void k_pcg_scalars(chol_pcg_rec *__restrict__ rec, const double *__restrict__ partial, int nb, int stride, int stage, double tol)
{
  __shared__ double s[2][256];
  const int j = blockIdx.x;
  const bool pair = stage == CHOL_PCG_STAGE_INIT || stage == CHOL_PCG_STAGE_VERIFY || stage == CHOL_PCG_STAGE_FINAL;
  const double *pp = partial + (int64_t)j * nb * stride;
  double sum = 0.0, sum2 = 0.0;
  for (int b0 = 0; b0 < nb; b0 += 256) {
    const int b = b0 + threadIdx.x, m = min(256, nb - b0);
    if (b < nb) { s[0][threadIdx.x] = pp[(int64_t)b * stride]; if (pair) s[1][threadIdx.x] = pp[(int64_t)b * stride + 1]; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll 8
      for (int k = 0; k < m; k++) sum += s[0][k];
      if (pair) {
#pragma unroll 8
        for (int k = 0; k < m; k++) sum2 += s[1][k];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  chol_pcg_rec c = rec[j];
  switch (stage) {
  case CHOL_PCG_STAGE_INIT: // sum = ||r||^2 of the start residual (the true one), sum2 = ||b||^2
    c.rho = c.sigma = c.alpha = c.beta = 0.0; c.iters = 0; c.what = 0;
    c.rr = sum; c.bb = sum2;
    c.rel = sum2 > 0.0 ? sqrt(sum / sum2) : sqrt(sum);
    if (!pcg_finite(sum) || !pcg_finite(sum2)) c.state = CHOL_PCG_NAN;
    else if (sum2 == 0.0) { c.state = CHOL_PCG_ZERO_B; c.rel = 0.0; }
    else c.state = c.rel <= tol ? CHOL_PCG_CONVERGED : CHOL_PCG_RESTART;
    break;
  case CHOL_PCG_STAGE_RHO: // sum = r^T z
    c.beta = 0.0;
    if (c.state == CHOL_PCG_RUNNING || c.state == CHOL_PCG_RESTART) {
      if (!pcg_finite(sum)) c.state = CHOL_PCG_NAN;
      else if (!(sum > 0.0)) { c.state = CHOL_PCG_BREAKDOWN; c.what = 1; }
      else { if (c.state == CHOL_PCG_RUNNING) c.beta = sum / c.rho; c.state = CHOL_PCG_RUNNING; } // (after a restart: p = z)
      c.rho = sum;
    }
    break;
  case CHOL_PCG_STAGE_SIGMA: // sum = p^T A p
    c.alpha = 0.0;
    if (c.state == CHOL_PCG_RUNNING) {
      c.iters++;
      c.sigma = sum;
      if (!pcg_finite(sum)) c.state = CHOL_PCG_NAN;
      else if (!(sum > 0.0)) { c.state = CHOL_PCG_BREAKDOWN; c.what = 2; }
      else c.alpha = c.rho / sum;
    }
    break;
  case CHOL_PCG_STAGE_RR: // sum = ||r||^2 of the recurrence
    c.alpha = 0.0;
    if (c.state == CHOL_PCG_RUNNING) {
      c.rr = sum;
      if (!pcg_finite(sum)) c.state = CHOL_PCG_NAN;
      else if (sum <= tol * tol * c.bb) c.state = CHOL_PCG_CLAIM;
    }
    break;
  case CHOL_PCG_STAGE_VERIFY: // sum = ||b - A x||^2 of a column that claims convergence
    if (c.state == CHOL_PCG_CLAIM) {
      c.rr = sum;
      c.rel = sqrt(sum / c.bb);
      c.state = !pcg_finite(sum) ? CHOL_PCG_NAN : c.rel <= tol ? CHOL_PCG_CONVERGED : CHOL_PCG_RESTART;
    }
    break;
  default: // FINAL: the true residual of what is returned
    if (c.state != CHOL_PCG_ZERO_B) c.rel = c.bb > 0.0 ? sqrt(sum / c.bb) : sqrt(sum);
    break;
  }
  rec[j] = c;
}
} // namespace

int chol_launch_pcg_apply(const int64_t *ptr, const int *col, const double *val, const double *P, int64_t ldp, double *Q, int64_t ldq, int n, int cols, double *partial, hipStream_t st)
{
  if (n <= 0 || cols <= 0) return 0;
  const int nb = (n + 255) / 256;
  // one column: the single-vector kernel; otherwise CHOL_PCG_APPLY_G columns per lane (the bits of a column are the same either way)
  if (cols == 1) hipLaunchKernelGGL((k_pcg_apply<1>), dim3(nb, 1), dim3(256), 0, st, ptr, col, val, P, ldp, Q, ldq, n, cols, partial);
  else hipLaunchKernelGGL((k_pcg_apply<CHOL_PCG_APPLY_G>), dim3(nb, (cols + CHOL_PCG_APPLY_G - 1) / CHOL_PCG_APPLY_G), dim3(256), 0, st, ptr, col, val, P, ldp, Q, ldq, n, cols, partial);
  return (int)hipGetLastError();
}
int chol_launch_pcg_update(const chol_pcg_rec *rec, const double *P, const double *Q, double *X, int64_t ldx, double *R, int64_t ld, int n, int cols, double *partial, hipStream_t st)
{
  if (n <= 0 || cols <= 0) return 0;
  hipLaunchKernelGGL(k_pcg_update, dim3((n + 255) / 256, cols), dim3(256), 0, st, rec, P, Q, X, ldx, R, ld, n, partial);
  return (int)hipGetLastError();
}
int chol_launch_pcg_dot(const double *R, const double *Z, int64_t ld, int n, int cols, double *partial, hipStream_t st)
{
  if (n <= 0 || cols <= 0) return 0;
  hipLaunchKernelGGL(k_pcg_dot, dim3((n + 255) / 256, cols), dim3(256), 0, st, R, Z, ld, n, partial);
  return (int)hipGetLastError();
}
int chol_launch_pcg_direction(const chol_pcg_rec *rec, const double *Z, double *P, int64_t ld, int n, int cols, hipStream_t st)
{
  if (n <= 0 || cols <= 0) return 0;
  hipLaunchKernelGGL(k_pcg_direction, dim3((n + 255) / 256, cols), dim3(256), 0, st, rec, Z, P, ld, n);
  return (int)hipGetLastError();
}
int chol_launch_pcg_take(const chol_pcg_rec *rec, const double *T, double *R, int64_t ld, int n, int cols, hipStream_t st)
{
  if (n <= 0 || cols <= 0) return 0;
  hipLaunchKernelGGL(k_pcg_take, dim3((n + 255) / 256, cols), dim3(256), 0, st, rec, T, R, ld, n);
  return (int)hipGetLastError();
}
int chol_launch_pcg_scalars(chol_pcg_rec *rec, const double *partial, int n, int cols, int stage, double tol, hipStream_t st)
{
  if (cols <= 0) return 0;
  const bool pair = stage == CHOL_PCG_STAGE_INIT || stage == CHOL_PCG_STAGE_VERIFY || stage == CHOL_PCG_STAGE_FINAL;
  hipLaunchKernelGGL(k_pcg_scalars, dim3(cols), dim3(256), 0, st, rec, partial, (n + 255) / 256, pair ? 2 : 1, stage, tol);
  return (int)hipGetLastError();
}
