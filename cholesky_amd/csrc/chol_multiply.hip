// Forward products with the factor: y = L z and y = L^T z in permuted coordinates (cholamd_multiply_half / cholamd_multiply and their _f32 forms), and the
// norms behind cholamd_factor_residual.  Input and output are distinct vectors, so there is no level chain: ONE launch covers the whole tree.  Its work
// list is chol_mul_lists (chol_plan.h): one workgroup per ITEM, an item owns 16 consecutive positions of the result and walks its sources in list order --
// one owner per output element, a fixed summation order, no floating-point atomics: two calls on one arena and one input return the same bits.
//
// Layout.  A panel is column-major, so 16 consecutive rows of one column are one 128-byte segment (64 bytes of an fp32 factor).  The 256 lanes form a
// 16 x 16 grid: `in` = lane & 15 runs along a column (stride 1), `out` = lane >> 4 across 16 columns (stride ld); every group of 16 lanes reads one whole
// segment per step (dwordx2 per lane), a wave four of them.
//   FORWARD   the item owns 16 ROWS: in = the row, out = the column modulo 16; a lane sums its row over the columns out, out + 16, ...
//   BACKWARD  the item owns 16 COLUMNS: out = the column, in = the row modulo 16; a lane sums its column over the rows in, in + 16, ...
// The reduction index advances in blocks of 256 steps whose z values are staged in LDS by one coalesced load (lane t brings z[z_off + block + t]); the 16
// loads of a block are issued back to back before the first multiply (16 segments in flight per lane group).  The 16 partial sums of every owned line are
// then added in a fixed order out of LDS.  Entries outside the lower triangle of a diagonal block and lines beyond the item's nv are never loaded: the
// upper triangles are not part of the factor and may hold anything.  The factor's element type is a template parameter; everything after the load is fp64.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "chol_kernels.h"

#define MUL_THREADS 256
#define MUL_STEPS (MUL_THREADS / CHOL_MUL_TILE) // reduction steps a lane takes per staged block of z
#define MUL_RED_LD (CHOL_MUL_TILE + 1)

template <class TL, int BW>
__global__ __launch_bounds__(MUL_THREADS) void k_multiply(const TL *__restrict__ base, const chol_mul_item *__restrict__ items, const chol_mul_src *__restrict__ srcs,
                                                          const double *__restrict__ z, double *__restrict__ y, const int *__restrict__ perm)
{
  __shared__ double zs[MUL_THREADS];
  __shared__ double red[CHOL_MUL_TILE * MUL_RED_LD]; // rows padded to 17: lanes that are 16 entries apart would share a bank
  const chol_mul_item it = items[blockIdx.x];
  const int t = threadIdx.x, in = t & (CHOL_MUL_TILE - 1), out = t >> 4;
  const int line = BW ? out : in;   // the owned line of this lane
  const int red0 = BW ? in : out;   // its place among the 16 lanes that share the line
  const bool owns = line < it.nv;
  double acc = 0.0;
  for (int s = it.src_first; s < it.src_end; s++) {
    const chol_mul_src q = srcs[s];
    // first / last reduction step this lane's line takes part in: the triangle of a diagonal block, everything elsewhere
    const int k_lo = BW ? max(q.tri + line, 0) : 0;
    const int k_hi = BW ? q.len : min(q.len, q.tri + line + 1);
    const TL *__restrict__ a = base + q.a_off + (BW ? (int64_t)line * q.ld : (int64_t)line);
    for (int kb = 0; kb < q.len; kb += MUL_THREADS) {
      __syncthreads(); // the previous block's zs are read
      zs[t] = kb + t < q.len ? z[q.z_off + kb + t] : 0.0;
      __syncthreads();
      double v[MUL_STEPS];
      bool ok[MUL_STEPS];
#pragma unroll
      for (int j = 0; j < MUL_STEPS; j++) {
        const int k = kb + j * CHOL_MUL_TILE + red0;
        ok[j] = owns && k >= k_lo && k < k_hi;
        v[j] = ok[j] ? (double)a[BW ? (int64_t)k : (int64_t)k * q.ld] : 0.0;
      }
#pragma unroll
      for (int j = 0; j < MUL_STEPS; j++)
        if (ok[j]) acc = fma(v[j], zs[j * CHOL_MUL_TILE + red0], acc);
    }
  }
  __syncthreads();
  red[line * MUL_RED_LD + red0] = acc;
  __syncthreads();
  if (t < it.nv) {
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < CHOL_MUL_TILE; j++) sum += red[t * MUL_RED_LD + j];
    const int pos = it.y_off + t;
    y[perm ? perm[pos] : pos] = sum;
  }
}

// ||A z - w||^2 and ||A z||^2 for w = M M^T z, A the device object's residual operator (CSR, both triangles, original dof order): one lane per row, one
// partial pair per workgroup by plain stores, a one-workgroup second stage in a fixed order -- the scheme of k_factor_logdet, no atomics.
// bad = rows where A z or w is not finite.
__global__ __launch_bounds__(MUL_THREADS) void k_multiply_resid(const int64_t *__restrict__ ptr, const int *__restrict__ col, const double *__restrict__ val,
                                                                const double *__restrict__ z, const double *__restrict__ w, int n, double *__restrict__ part, long long *__restrict__ ipart)
{
  __shared__ double sd[MUL_THREADS], sa[MUL_THREADS];
  __shared__ long long sb[MUL_THREADS];
  const int i = blockIdx.x * MUL_THREADS + threadIdx.x, t = threadIdx.x;
  double d2 = 0.0, a2 = 0.0;
  long long bad = 0;
  if (i < n) {
    double az = 0.0;
    for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) az = fma(val[e], z[col[e]], az);
    const double d = az - w[i];
    if (fabs(az) <= DBL_MAX && fabs(d) <= DBL_MAX) { d2 = d * d; a2 = az * az; } // (NaN fails both)
    else bad = 1;
  }
  sd[t] = d2; sa[t] = a2; sb[t] = bad;
  __syncthreads();
  for (int o = MUL_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) { sd[t] += sd[t + o]; sa[t] += sa[t + o]; sb[t] += sb[t + o]; }
    __syncthreads();
  }
  if (t == 0) { part[2 * blockIdx.x] = sd[0]; part[2 * blockIdx.x + 1] = sa[0]; ipart[blockIdx.x] = sb[0]; }
}
__global__ __launch_bounds__(MUL_THREADS) void k_multiply_resid_sum(const double *__restrict__ part, const long long *__restrict__ ipart, int nblk, long long *__restrict__ res)
{
  __shared__ double sd[MUL_THREADS], sa[MUL_THREADS];
  __shared__ long long sb[MUL_THREADS];
  const int t = threadIdx.x;
  double d2 = 0.0, a2 = 0.0;
  long long bad = 0;
  for (int b = t; b < nblk; b += MUL_THREADS) { d2 += part[2 * b]; a2 += part[2 * b + 1]; bad += ipart[b]; }
  sd[t] = d2; sa[t] = a2; sb[t] = bad;
  __syncthreads();
  for (int o = MUL_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) { sd[t] += sd[t + o]; sa[t] += sa[t + o]; sb[t] += sb[t + o]; }
    __syncthreads();
  }
  if (t == 0) { res[0] = __double_as_longlong(sd[0]); res[1] = __double_as_longlong(sa[0]); res[2] = sb[0]; }
}

template <class TL>
int chol_launch_multiply(const TL *base, const chol_mul_item *items, int n_items, const chol_mul_src *srcs, int backward, const double *z, double *y, const int *perm, hipStream_t st)
{
  if (n_items <= 0) return 0;
  if (backward) hipLaunchKernelGGL((k_multiply<TL, 1>), dim3(n_items), dim3(MUL_THREADS), 0, st, base, items, srcs, z, y, perm);
  else hipLaunchKernelGGL((k_multiply<TL, 0>), dim3(n_items), dim3(MUL_THREADS), 0, st, base, items, srcs, z, y, perm);
  return (int)hipGetLastError();
}

template int chol_launch_multiply(const double *, const chol_mul_item *, int, const chol_mul_src *, int, const double *, double *, const int *, hipStream_t);
template int chol_launch_multiply(const float *, const chol_mul_item *, int, const chol_mul_src *, int, const double *, double *, const int *, hipStream_t);
int chol_launch_multiply_resid(const int64_t *ptr, const int *col, const double *val, const double *z, const double *w, int n, double *part, int64_t *ipart, int64_t *res, hipStream_t st)
{
  const int nblk = n > 0 ? (n + MUL_THREADS - 1) / MUL_THREADS : 0;
  if (nblk > 0) {
    hipLaunchKernelGGL(k_multiply_resid, dim3(nblk), dim3(MUL_THREADS), 0, st, ptr, col, val, z, w, n, part, (long long *)ipart);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(k_multiply_resid_sum, dim3(1), dim3(MUL_THREADS), 0, st, part, (const long long *)ipart, nblk, (long long *)res);
  return (int)hipGetLastError();
}
