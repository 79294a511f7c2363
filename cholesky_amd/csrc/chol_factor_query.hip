// Factor queries: the diagonal of L and log det A = 2 sum_i log L_ii, read straight from the arena (cholamd_factor_diag / cholamd_factor_logdet and their
// _f32 forms).  One launch walks the diagonal of the whole tree: the TRSV descriptors of every level, concatenated and ordered by permuted position
// (chol_diag_list), with a prefix array of column counts that a lane searches for its position.  Element j of descriptor s is base[a_off + j (lda + 1)]:
// every read touches a sector of its own, n x 64 B in all; nothing is staged.  The factor's element type is a template parameter (fp64 / fp32 arena);
// everything after the load is fp64.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "chol_kernels.h"

#define FQ_THREADS 256
#define FQ_WAVES (FQ_THREADS / 64)
#define FQ_NONE 0x7fffffffffffffffLL

// entry i of the walk: L(pos, pos) as fp64 and its permuted position
template <class TL>
__device__ __forceinline__ double fq_entry(const TL *__restrict__ base, const chol_trsv_desc *__restrict__ descs, const int *__restrict__ prefix, int nd, int i, int *pos)
{
  int lo = 0, hi = nd - 1; // the last descriptor with prefix[s] <= i (empty descriptors share their successor's prefix and are passed over)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= i) lo = mid; else hi = mid - 1;
  }
  const int j = i - prefix[lo];
  *pos = descs[lo].x_off + j;
  return (double)base[descs[lo].a_off + (int64_t)j * (descs[lo].lda + 1)];
}

// The sum of the logs is carried as an unevaluated pair hi + lo (error-free TwoSum at every addition, additions only: nothing for the compiler to
// contract), from the lanes through the wave and workgroup reductions and the partials to the final result: hi + lo is the correctly rounded sum of the
// fp64 logs in all but boundary cases, whatever n -- 2 sum log d_diag summed exactly on the host reproduces it.
struct fq_dd { double hi, lo; };
__device__ __forceinline__ void fq_add(fq_dd &a, double x, double xlo = 0.0)
{
  const double s = a.hi + x, bb = s - a.hi;
  a.lo += ((a.hi - (s - bb)) + (x - bb)) + xlo;
  a.hi = s;
}

template <class TL>
__global__ __launch_bounds__(FQ_THREADS) void k_factor_diag(const TL *__restrict__ base, const chol_trsv_desc *__restrict__ descs, const int *__restrict__ prefix, int nd, int n,
                                                            const int *__restrict__ perm, double *__restrict__ diag)
{
  const int i = blockIdx.x * FQ_THREADS + threadIdx.x;
  if (i >= n) return;
  int pos;
  const double v = fq_entry(base, descs, prefix, nd, i, &pos);
  diag[perm[pos]] = v; // original dof order
}

// stage 1: a fixed assignment of entries to lanes (grid-stride), a fixed reduction tree inside the workgroup, one partial per workgroup by a plain store
template <class TL>
__global__ __launch_bounds__(FQ_THREADS) void k_factor_logdet(const TL *__restrict__ base, const chol_trsv_desc *__restrict__ descs, const int *__restrict__ prefix, int nd, int n,
                                                              double *__restrict__ part, long long *__restrict__ ipart)
{
  __shared__ double ssum[FQ_WAVES], slo[FQ_WAVES];
  __shared__ long long sbad[FQ_WAVES], sfirst[FQ_WAVES];
  fq_dd acc = { 0.0, 0.0 };
  long long nbad = 0, first = FQ_NONE;
  for (int i = blockIdx.x * FQ_THREADS + threadIdx.x; i < n; i += gridDim.x * FQ_THREADS) {
    int pos;
    const double v = fq_entry(base, descs, prefix, nd, i, &pos);
    if (v > 0.0 && v <= DBL_MAX) fq_add(acc, log(v)); // (NaN fails both)
    else { nbad++; first = pos < first ? pos : first; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double h = __shfl_down(acc.hi, o, 64), l = __shfl_down(acc.lo, o, 64);
    fq_add(acc, h, l);
    nbad += __shfl_down(nbad, o, 64);
    const long long f = __shfl_down(first, o, 64);
    first = f < first ? f : first;
  }
  if ((threadIdx.x & 63) == 0) { ssum[threadIdx.x >> 6] = acc.hi; slo[threadIdx.x >> 6] = acc.lo; sbad[threadIdx.x >> 6] = nbad; sfirst[threadIdx.x >> 6] = first; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < FQ_WAVES; w++) { fq_add(acc, ssum[w], slo[w]); nbad += sbad[w]; first = sfirst[w] < first ? sfirst[w] : first; }
    part[2 * blockIdx.x] = acc.hi;
    part[2 * blockIdx.x + 1] = acc.lo;
    ipart[2 * blockIdx.x] = nbad;
    ipart[2 * blockIdx.x + 1] = first;
  }
}

// stage 2, one workgroup: lane t sums the partials t, t + 256, ... , then a pairwise tree over the lanes in LDS -- the same order on every call
__global__ __launch_bounds__(FQ_THREADS) void k_factor_logdet_sum(const double *__restrict__ part, const long long *__restrict__ ipart, int nblk, long long *__restrict__ res)
{
  __shared__ double ssum[FQ_THREADS], slo[FQ_THREADS];
  __shared__ long long sbad[FQ_THREADS], sfirst[FQ_THREADS];
  fq_dd s = { 0.0, 0.0 };
  long long nbad = 0, first = FQ_NONE;
  for (int b = threadIdx.x; b < nblk; b += FQ_THREADS) {
    fq_add(s, part[2 * b], part[2 * b + 1]);
    nbad += ipart[2 * b];
    first = ipart[2 * b + 1] < first ? ipart[2 * b + 1] : first;
  }
  ssum[threadIdx.x] = s.hi; slo[threadIdx.x] = s.lo; sbad[threadIdx.x] = nbad; sfirst[threadIdx.x] = first;
  __syncthreads();
  for (int o = FQ_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      fq_dd t = { ssum[threadIdx.x], slo[threadIdx.x] };
      fq_add(t, ssum[threadIdx.x + o], slo[threadIdx.x + o]);
      ssum[threadIdx.x] = t.hi; slo[threadIdx.x] = t.lo;
      sbad[threadIdx.x] += sbad[threadIdx.x + o];
      if (sfirst[threadIdx.x + o] < sfirst[threadIdx.x]) sfirst[threadIdx.x] = sfirst[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    res[0] = __double_as_longlong(2.0 * (ssum[0] + slo[0]));
    res[1] = sbad[0];
    res[2] = sfirst[0];
  }
}

template <class TL>
int chol_launch_factor_diag(const TL *base, const chol_trsv_desc *descs, const int *prefix, int nd, int n, const int *perm, double *diag, hipStream_t st)
{
  if (n <= 0 || nd <= 0) return 0;
  hipLaunchKernelGGL(k_factor_diag<TL>, dim3((n + FQ_THREADS - 1) / FQ_THREADS), dim3(FQ_THREADS), 0, st, base, descs, prefix, nd, n, perm, diag);
  return (int)hipGetLastError();
}
template <class TL>
int chol_launch_factor_logdet(const TL *base, const chol_trsv_desc *descs, const int *prefix, int nd, int n, double *part, int64_t *ipart, int64_t *res, hipStream_t st)
{
  int nblk = (n + FQ_THREADS - 1) / FQ_THREADS;
  if (nblk > CHOL_LOGDET_MAX_BLOCKS) nblk = CHOL_LOGDET_MAX_BLOCKS;
  if (nblk < 1 || nd <= 0) nblk = 0; // an empty system: log det = 0
  if (nblk > 0) {
    hipLaunchKernelGGL(k_factor_logdet<TL>, dim3(nblk), dim3(FQ_THREADS), 0, st, base, descs, prefix, nd, n, part, (long long *)ipart);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(k_factor_logdet_sum, dim3(1), dim3(FQ_THREADS), 0, st, part, (const long long *)ipart, nblk, (long long *)res);
  return (int)hipGetLastError();
}

template int chol_launch_factor_diag(const double *, const chol_trsv_desc *, const int *, int, int, const int *, double *, hipStream_t);
template int chol_launch_factor_diag(const float *, const chol_trsv_desc *, const int *, int, int, const int *, double *, hipStream_t);
template int chol_launch_factor_logdet(const double *, const chol_trsv_desc *, const int *, int, int, double *, int64_t *, int64_t *, hipStream_t);
template int chol_launch_factor_logdet(const float *, const chol_trsv_desc *, const int *, int, int, double *, int64_t *, int64_t *, hipStream_t);
