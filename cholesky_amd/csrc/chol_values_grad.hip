// Gradients with respect to the value array (cholamd_values_grad_pairs, cholamd_values_grad_logdet): the contraction of an adjoint onto the entries of
// A(v) = sum_k v_k E_k, E_k = e_i e_j^T + e_j e_i^T off the diagonal and e_i e_i^T on it, (i, j) = entry k of the plan's entry list.
//
//   pairs    g[k] = alpha s_k + beta g[k],  s_k = sum_c p_c^T E_k q_c      P, Q column-major n x nrhs in original dof order
//   logdet   g[k] = alpha t_k + beta g[k],  t_k = tr(A^-1 E_k) = m_k Z(i, j)  Z the arena of cholamd_selinv, m_k = 2 off the diagonal, 1 on it
//
// Entries outside the pattern (CHOL_ENTRY_OUT) have s_k = t_k = 0: g[k] = beta g[k].  beta == 0: g is never read (0.0 for those entries).
// One owner per entry, plain stores, no atomics and no waits between workgroups; the order of the sum is fixed (the host restatements in
// chol_symbolic.c repeat it with fma() to the bit): acc = 0; for c ascending: acc = fma(P[i,c], Q[j,c], acc); off the diagonal then
// acc = fma(P[j,c], Q[i,c], acc); at the end g = beta == 0 ? alpha acc : fma(alpha, acc, beta g).
//
// Lanes lie across consecutive entries and each runs the column loop.  The entry lists the project produces are sorted by column, so neighbouring lanes
// read neighbouring rows of P and Q (the row streams of a stencil), and a column of P and Q is 8 n bytes that stay in L2 while the workgroups pass over
// it.  The kernel is bound by the latency of those gathers: the loop is unrolled by four columns so that sixteen independent loads are in flight per
// lane before the first fma of the chain needs one (the fmas themselves stay in order).
#include <hip/hip_runtime.h>

#include "chol_kernels.h"

#ifndef VG_THREADS
#define VG_THREADS 256 // entries per workgroup, one per lane
#endif
#ifndef VG_UNROLL
#define VG_UNROLL 4    // columns whose loads are issued before the first fma
#endif

__device__ __forceinline__ double vg_scale(double alpha, double t, double beta, const double *g) // beta == 0: *g is not read
{
  return beta == 0.0 ? alpha * t : fma(alpha, t, beta * *g);
}

__global__ __launch_bounds__(VG_THREADS) void k_values_grad_pairs(const double *__restrict__ P, int64_t ldp, const double *__restrict__ Q, int64_t ldq, int nrhs,
                                                                  const int *__restrict__ e_row, const int *__restrict__ e_col, const unsigned char *__restrict__ e_cls,
                                                                  int64_t nz, double alpha, double beta, double *g)
{
  const int64_t k = (int64_t)blockIdx.x * VG_THREADS + threadIdx.x;
  if (k >= nz) return;
  if (e_cls[k] != CHOL_ENTRY_IN) { g[k] = beta == 0.0 ? 0.0 : beta * g[k]; return; } // A(v) does not depend on v_k
  const int64_t i = e_row[k], j = e_col[k];
  const double *Pi = P + i, *Pj = P + j, *Qi = Q + i, *Qj = Q + j;
  double acc = 0.0;
  int c = 0;
  if (i != j) {
    for (; c + VG_UNROLL <= nrhs; c += VG_UNROLL) {
      double pi[VG_UNROLL], pj[VG_UNROLL], qi[VG_UNROLL], qj[VG_UNROLL];
#pragma unroll
      for (int u = 0; u < VG_UNROLL; u++) {
        const int64_t op = (int64_t)(c + u) * ldp, oq = (int64_t)(c + u) * ldq;
        pi[u] = Pi[op]; qj[u] = Qj[oq]; pj[u] = Pj[op]; qi[u] = Qi[oq];
      }
#pragma unroll
      for (int u = 0; u < VG_UNROLL; u++) { acc = fma(pi[u], qj[u], acc); acc = fma(pj[u], qi[u], acc); }
    }
    for (; c < nrhs; c++) {
      const int64_t op = (int64_t)c * ldp, oq = (int64_t)c * ldq;
      acc = fma(Pi[op], Qj[oq], acc);
      acc = fma(Pj[op], Qi[oq], acc);
    }
  } else {
    for (; c + VG_UNROLL <= nrhs; c += VG_UNROLL) {
      double pi[VG_UNROLL], qi[VG_UNROLL];
#pragma unroll
      for (int u = 0; u < VG_UNROLL; u++) { pi[u] = Pi[(int64_t)(c + u) * ldp]; qi[u] = Qi[(int64_t)(c + u) * ldq]; }
#pragma unroll
      for (int u = 0; u < VG_UNROLL; u++) acc = fma(pi[u], qi[u], acc);
    }
    for (; c < nrhs; c++) acc = fma(Pi[(int64_t)c * ldp], Qi[(int64_t)c * ldq], acc);
  }
  g[k] = vg_scale(alpha, acc, beta, &g[k]);
}

// threads [0, nz): the entries outside the pattern; threads [nz, nz + nnz): scatter entry e = thread - nz owns g[a_src[e]] (no two entries of a plan the
// call accepts share a position, so no k has two writers)
__global__ __launch_bounds__(VG_THREADS) void k_values_grad_logdet(const double *__restrict__ Z, const int64_t *__restrict__ a_dst, const int *__restrict__ a_src, int64_t nnz,
                                                                   const int *__restrict__ e_row, const int *__restrict__ e_col, const unsigned char *__restrict__ e_cls,
                                                                   int64_t nz, double alpha, double beta, double *g)
{
  const int64_t t = (int64_t)blockIdx.x * VG_THREADS + threadIdx.x;
  if (t < nz) {
    if (e_cls[t] != CHOL_ENTRY_IN) g[t] = beta == 0.0 ? 0.0 : beta * g[t];
    return;
  }
  const int64_t e = t - nz;
  if (e >= nnz) return;
  const int k = a_src[e];
  const double m = e_row[k] == e_col[k] ? 1.0 : 2.0;
  g[k] = vg_scale(alpha, m * Z[a_dst[e]], beta, &g[k]);
}

int chol_launch_values_grad_pairs(const double *P, int64_t ldp, const double *Q, int64_t ldq, int nrhs, const int *e_row, const int *e_col, const unsigned char *e_cls,
                                  int64_t nz, double alpha, double beta, double *g, hipStream_t st)
{
  if (nz <= 0) return 0;
  hipLaunchKernelGGL(k_values_grad_pairs, dim3((unsigned)((nz + VG_THREADS - 1) / VG_THREADS)), dim3(VG_THREADS), 0, st, P, ldp, Q, ldq, nrhs, e_row, e_col, e_cls, nz,
                     alpha, beta, g);
  return (int)hipGetLastError();
}
int chol_launch_values_grad_logdet(const double *Z, const int64_t *a_dst, const int *a_src, int64_t nnz, const int *e_row, const int *e_col, const unsigned char *e_cls,
                                   int64_t nz, double alpha, double beta, double *g, hipStream_t st)
{
  if (nz <= 0) return 0;
  hipLaunchKernelGGL(k_values_grad_logdet, dim3((unsigned)((nz + nnz + VG_THREADS - 1) / VG_THREADS)), dim3(VG_THREADS), 0, st, Z, a_dst, a_src, nnz, e_row, e_col, e_cls,
                     nz, alpha, beta, g);
  return (int)hipGetLastError();
}
