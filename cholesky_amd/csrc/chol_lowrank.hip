// Tall-skinny dense kernels of the low-rank corrections (cholamd_lowrank_*; include/cholamd.h at "low-rank corrections", partition in chol_plan.h at
// CHOL_LR_SLAB).  fp64 throughout, column-major blocks with leading dimensions, n rows (millions), k <= CHOL_LR_MAX columns.  Every kernel is a plain grid:
// one owner per output element, sums in a fixed order, no floating-point atomics, no flags, no waits inside a launch; stages are ordered by kernel
// boundaries on the stream alone.  Two calls return the same bits.
//
//   k_lr_tprod / k_lr_tsum   T = P^T Q (k x m), the Gram matrix P^T P with its lower tiles only, mirrored on write
//   k_lr_rprod               X = alpha X + beta V T (n x m), rows owned in chunks of 16: X == V (m == k) is legal
//   k_lr_rprod32             the same for m <= 32, the reduction shared by the four waves
//   k_lr_rowsq               w_i = sum_j W_ij^2
//
// v_mfma_f64_16x16x4_f64: lane l holds A(l & 15, l >> 4) and B(l >> 4, l & 15); result register q: row (l >> 4) + 4 q, column l & 15.
//   tprod   A(i, r) = P(row r, column i), B(r, j) = Q(row r, column j), both out of the LDS image of CHOL_LR_STAGE rows: image[column][row] with rows padded to
//           CHOL_LR_STAGE + 2, so that the 32 lanes of a ds_read_b64 half (16 columns x 2 rows) fall on 32 different bank pairs; the image is written with
//           consecutive lanes along a column (256 contiguous bytes of HBM per 32 lanes)
//   rprod   the TRANSPOSED tile X^T = T^T V^T: A(j, c) = T(c, j), B(c, i) = V(row i, column c) out of the chunk's LDS image -- the result's column index (the
//           16 consecutive lanes) is then the ROW of X, and a store is 128 contiguous bytes of a column of X
// Ragged n, k, m: an operand that is not meant is read CLAMPED inside its block and SELECTED to 0.0, never multiplied by zero; what lies behind a
// block's end or in another column may be NaN.  Results outside n x m are not written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chol_kernels.h"
#include "chol_plan.h"

#define LR_THREADS (64 * CHOL_LR_WAVES)
#define LR_LD (CHOL_LR_STAGE + 2)
#define LR_STEPS (CHOL_LR_STAGE / 4)
#define LRR_THREADS (64 * CHOL_LR_RWAVES)
static_assert(CHOL_LR_MAX % 16 == 0 && CHOL_LR_STAGE == 32 && CHOL_LR_SLAB % CHOL_LR_STAGE == 0 && CHOL_LR_ROWS == 16, "16 x 16 tiles, 32 staged rows");
static_assert(CHOL_LR_SLOTS * CHOL_LR_WAVES >= (CHOL_LR_MAX / 16) * (CHOL_LR_MAX / 16 + 1) / 2 && CHOL_LR_SLOTS * CHOL_LR_WAVES >= (CHOL_LR_MAX / 16) * (CHOL_NRHS_W / 16),
              "every tile of a call has an owner");

typedef double ld4 __attribute__((ext_vector_type(4)));

// image[c * LR_LD + r] = B(r0 + r, c) for c < ct * 16, r < CHOL_LR_STAGE; 0.0 where the row is >= rend or the column >= cols
__device__ __forceinline__ void lr_stage(double *image, const double *__restrict__ B, int64_t ld, int64_t n, int cols, int ct, int64_t r0, int64_t rend, int t)
{
  for (int e = t; e < ct * 16 * CHOL_LR_STAGE; e += LR_THREADS) {
    const int r = e & (CHOL_LR_STAGE - 1), c = e / CHOL_LR_STAGE;
    const int64_t row = r0 + r;
    const double v = B[(row < n ? row : n - 1) + (int64_t)(c < cols ? c : cols - 1) * ld];
    image[c * LR_LD + r] = (row < rend && c < cols) ? v : 0.0;
  }
}

// stage 1: workgroup = slab.  ws[(slab * ntiles + id) * 256 + row * 16 + column] = the slab's partial of tile id
template <bool GRAM>
__global__ __launch_bounds__(LR_THREADS) void k_lr_tprod(int64_t n, int k, int m, const double *__restrict__ P, int64_t ldp, const double *__restrict__ Q, int64_t ldq, double *__restrict__ ws)
{
  __shared__ double Ps[CHOL_LR_MAX * LR_LD];
  __shared__ double Qs[GRAM ? 1 : CHOL_NRHS_W * LR_LD];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i16 = lane & 15, g = lane >> 4;
  const int kt = (k + 15) / 16, mt = (m + 15) / 16, ntiles = GRAM ? chol_lr_gram_tiles(kt) : kt * mt;
  const int64_t slab0 = (int64_t)blockIdx.x * CHOL_LR_SLAB, rend = slab0 + CHOL_LR_SLAB < n ? slab0 + CHOL_LR_SLAB : n;
  int ti[CHOL_LR_SLOTS], tj[CHOL_LR_SLOTS];
  ld4 acc[CHOL_LR_SLOTS];
#pragma unroll
  for (int s = 0; s < CHOL_LR_SLOTS; ++s) {
    const int id = wave + s * CHOL_LR_WAVES;
    int a = 0, b = 0;
    if (id < ntiles) { if (GRAM) chol_lr_gram_tile(id, &a, &b); else { a = id / mt; b = id % mt; } }
    ti[s] = __builtin_amdgcn_readfirstlane(a); tj[s] = __builtin_amdgcn_readfirstlane(b);
    acc[s] = ld4{ 0.0, 0.0, 0.0, 0.0 };
  }
  const double *Bs = GRAM ? Ps : Qs;
  for (int64_t r0 = slab0; r0 < rend; r0 += CHOL_LR_STAGE) {
    __syncthreads(); // the image's readers of the block before
    lr_stage(Ps, P, ldp, n, k, kt, r0, rend, t);
    if (!GRAM) lr_stage(Qs, Q, ldq, n, m, mt, r0, rend, t);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < CHOL_LR_SLOTS; ++s) {
      if (wave + s * CHOL_LR_WAVES < ntiles) { // (wave-uniform)
        const double *pa = Ps + (ti[s] * 16 + i16) * LR_LD + g, *pb = Bs + (tj[s] * 16 + i16) * LR_LD + g;
#pragma unroll
        for (int u = 0; u < LR_STEPS; ++u) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[4 * u], pb[4 * u], acc[s], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < CHOL_LR_SLOTS; ++s) {
    const int id = wave + s * CHOL_LR_WAVES;
    if (id < ntiles) {
      double *out = ws + ((int64_t)blockIdx.x * ntiles + id) * 256;
#pragma unroll
      for (int q = 0; q < 4; ++q) out[(g + 4 * q) * 16 + i16] = acc[s][q];
    }
  }
}

// stage 2: workgroup = tile, thread = element; the slabs' partials in slab order.  gram: the tile's mirror image is written too
__global__ __launch_bounds__(256) void k_lr_tsum(const double *__restrict__ ws, int64_t nslab, int ntiles, int gram, int k, int m, double *__restrict__ T, int64_t ldt)
{
  const int id = blockIdx.x, e = threadIdx.x, mt = (m + 15) / 16;
  int ti, tj;
  if (gram) chol_lr_gram_tile(id, &ti, &tj); else { ti = id / mt; tj = id % mt; }
  double sum = ws[(int64_t)id * 256 + e];
  for (int64_t s = 1; s < nslab; ++s) sum += ws[(s * ntiles + id) * 256 + e];
  const int i = ti * 16 + (e >> 4), j = tj * 16 + (e & 15);
  if (i < k && j < m) {
    T[i + (int64_t)j * ldt] = sum;
    if (gram && ti != tj) T[j + (int64_t)i * ldt] = sum;
  }
}

// workgroup = the rows [16 b, 16 b + 16): all of them read into LDS (and nothing written) before the first store; a wave reads an element of X only just
// before it writes that element
__global__ __launch_bounds__(LRR_THREADS) void k_lr_rprod(int64_t n, int k, int m, double alpha, double beta, const double *V, int64_t ldv, const double *__restrict__ T, int64_t ldt,
                                                          double *X, int64_t ldx)
{
  extern __shared__ double Vs[]; // [column][row], columns padded to a multiple of 4
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i16 = lane & 15, g = lane >> 4, k4 = (k + 3) & ~3;
  const int64_t r0 = (int64_t)blockIdx.x * CHOL_LR_ROWS, row = r0 + i16;
  for (int e = t; e < k4 * CHOL_LR_ROWS; e += LRR_THREADS) {
    const int r = e & (CHOL_LR_ROWS - 1), c = e / CHOL_LR_ROWS;
    const double v = V[(r0 + r < n ? r0 + r : n - 1) + (int64_t)(c < k ? c : k - 1) * ldv];
    Vs[e] = (r0 + r < n && c < k) ? v : 0.0;
  }
  __syncthreads();
  for (int c0 = wave * CHOL_NRHS_W; c0 < m; c0 += CHOL_LR_RWAVES * CHOL_NRHS_W) {
    const int j0 = c0 + i16, j1 = j0 + 16;
    const double *t0 = T + (int64_t)(j0 < m ? j0 : m - 1) * ldt, *t1 = T + (int64_t)(j1 < m ? j1 : m - 1) * ldt;
    ld4 acc0 = { 0.0, 0.0, 0.0, 0.0 }, acc1 = { 0.0, 0.0, 0.0, 0.0 };
    for (int cb = 0; cb < k4; cb += 4) { // (uniform: every lane of the wave takes part in every MFMA)
      const int c = cb + g, cc = c < k ? c : k - 1;
      const double v0 = t0[cc], v1 = t1[cc], b = Vs[c * CHOL_LR_ROWS + i16];
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64((c < k && j0 < m) ? v0 : 0.0, b, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64((c < k && j1 < m) ? v1 : 0.0, b, acc1, 0, 0, 0);
    }
    if (row < n) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = c0 + 16 * h + g + 4 * q;
          if (j < m) {
            double *x = X + row + (int64_t)j * ldx;
            const double p = beta * (h ? acc1[q] : acc0[q]);
            *x = alpha != 0.0 ? alpha * *x + p : p;
          }
        }
    }
  }
}

// The same product for a call of at most 32 columns (the corrected solves: X -= sigma W t): the reduction over V's columns is cut into four consecutive
// ranges of MFMA steps, one per wave -- a partition of k alone -- so the four waves share the call's only column tile pair; a wave fetches its operands
// of T before the stage barrier, keeps one 32 x 16 partial tile, and the four tiles are added in wave order out of LDS by the element's owner
// (consecutive lanes along a column of X).  The chunk's rows of V are in LDS before the first store and an element of X is read by its owner alone, so
// X == V stays legal here too.
#define LRR_USTEPS (CHOL_LR_MAX / 4 / CHOL_LR_RWAVES)
__global__ __launch_bounds__(LRR_THREADS) void k_lr_rprod32(int64_t n, int k, int m, double alpha, double beta, const double *V, int64_t ldv, const double *__restrict__ T, int64_t ldt,
                                                            double *X, int64_t ldx)
{
  extern __shared__ double Vs[]; // [column][row], columns padded to a multiple of 4
  __shared__ double red[CHOL_LR_RWAVES * CHOL_NRHS_W * CHOL_LR_ROWS];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i16 = lane & 15, g = lane >> 4, k4 = (k + 3) & ~3;
  const int steps = k4 / 4, sw = (steps + CHOL_LR_RWAVES - 1) / CHOL_LR_RWAVES, s0 = wave * sw, s1 = s0 + sw < steps ? s0 + sw : steps;
  const int64_t r0 = (int64_t)blockIdx.x * CHOL_LR_ROWS;
  const int j0 = i16, j1 = 16 + i16;
  const double *t0 = T + (int64_t)(j0 < m ? j0 : m - 1) * ldt, *t1 = T + (int64_t)(j1 < m ? j1 : m - 1) * ldt;
  double a0[LRR_USTEPS], a1[LRR_USTEPS];
#pragma unroll
  for (int u = 0; u < LRR_USTEPS; ++u) {
    const int c = 4 * (s0 + u) + g, cc = c < k ? c : k - 1;
    const double v0 = t0[cc], v1 = t1[cc];
    a0[u] = (c < k && j0 < m) ? v0 : 0.0;
    a1[u] = (c < k && j1 < m) ? v1 : 0.0;
  }
  for (int e = t; e < k4 * CHOL_LR_ROWS; e += LRR_THREADS) {
    const int r = e & (CHOL_LR_ROWS - 1), c = e / CHOL_LR_ROWS;
    const double v = V[(r0 + r < n ? r0 + r : n - 1) + (int64_t)(c < k ? c : k - 1) * ldv];
    Vs[e] = (r0 + r < n && c < k) ? v : 0.0;
  }
  __syncthreads();
  ld4 acc0 = { 0.0, 0.0, 0.0, 0.0 }, acc1 = { 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
  for (int u = 0; u < LRR_USTEPS; ++u)
    if (s0 + u < s1) { // (wave-uniform; the image ends at step `steps`)
      const double b = Vs[(4 * (s0 + u) + g) * CHOL_LR_ROWS + i16];
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u], b, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[u], b, acc1, 0, 0, 0);
    }
  double *mine = red + wave * (CHOL_NRHS_W * CHOL_LR_ROWS);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    mine[(g + 4 * q) * CHOL_LR_ROWS + i16] = acc0[q];
    mine[(16 + g + 4 * q) * CHOL_LR_ROWS + i16] = acc1[q];
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int e = t + h * LRR_THREADS, r = e & (CHOL_LR_ROWS - 1), j = e / CHOL_LR_ROWS;
    double sum = red[e];
#pragma unroll
    for (int w = 1; w < CHOL_LR_RWAVES; ++w) sum += red[w * (CHOL_NRHS_W * CHOL_LR_ROWS) + e];
    if (r0 + r < n && j < m) {
      double *x = X + r0 + r + (int64_t)j * ldx;
      const double p = beta * sum;
      *x = alpha != 0.0 ? alpha * *x + p : p;
    }
  }
}
static_assert(LRR_USTEPS * CHOL_LR_RWAVES * 4 == CHOL_LR_MAX && 2 * LRR_THREADS == CHOL_NRHS_W * CHOL_LR_ROWS, "a wave's steps, two results per lane");

__global__ __launch_bounds__(256) void k_lr_rowsq(int64_t n, int k, const double *__restrict__ W, int64_t ldw, double *__restrict__ w)
{
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int j = 0; j < k; ++j) { const double v = W[i + (int64_t)j * ldw]; s += v * v; }
  w[i] = s;
}

// the k x k helpers of cholamd_lowrank_set and of the constraint right-hand side: what = 0: C = I + mode G in place (mode 0: C = G); 1: the identity;
// 2: A(:, j) -= B(:, j) for j < cols
__global__ __launch_bounds__(256) void k_lr_small(int what, int k, int cols, int mode, double *__restrict__ A, int64_t lda, const double *__restrict__ B, int64_t ldb)
{
  const int e = blockIdx.x * 256 + threadIdx.x, i = e % k, j = e / k;
  if (j >= cols) return;
  double *a = A + i + (int64_t)j * lda;
  if (what == 0) *a = mode == 0 ? *a : (i == j ? 1.0 : 0.0) + (mode > 0 ? *a : -*a);
  else if (what == 1) *a = i == j ? 1.0 : 0.0;
  else *a -= B[i + (int64_t)j * ldb];
}

int64_t chol_lr_ws_doubles(int64_t n, int kmax)
{
  const int kt = (kmax + 15) / 16, gram = chol_lr_gram_tiles(kt), gen = kt * (CHOL_NRHS_W / 16);
  return chol_lr_slabs(n) * (gram > gen ? gram : gen) * 256;
}

int chol_launch_lr_tprod(int64_t n, int k, int m, const double *P, int64_t ldp, const double *Q, int64_t ldq, double *ws, double *T, int64_t ldt, hipStream_t st)
{
  if (n <= 0 || k <= 0 || m <= 0) return 0;
  if (k > CHOL_LR_MAX) return (int)hipErrorInvalidValue; // the LDS image holds CHOL_LR_MAX columns
  const int kt = (k + 15) / 16;
  const int64_t nslab = chol_lr_slabs(n);
  if (P == Q && ldp == ldq && m == k) {
    const int ntiles = chol_lr_gram_tiles(kt);
    hipLaunchKernelGGL((k_lr_tprod<true>), dim3((unsigned)nslab), dim3(LR_THREADS), 0, st, n, k, k, P, ldp, P, ldp, ws);
    hipLaunchKernelGGL(k_lr_tsum, dim3(ntiles), dim3(256), 0, st, ws, nslab, ntiles, 1, k, k, T, ldt);
    return (int)hipGetLastError();
  }
  for (int c0 = 0; c0 < m; c0 += CHOL_NRHS_W) { // a column's partition does not depend on its chunk
    const int cols = m - c0 < CHOL_NRHS_W ? m - c0 : CHOL_NRHS_W, ntiles = kt * ((cols + 15) / 16);
    hipLaunchKernelGGL((k_lr_tprod<false>), dim3((unsigned)nslab), dim3(LR_THREADS), 0, st, n, k, cols, P, ldp, Q + (int64_t)c0 * ldq, ldq, ws);
    hipLaunchKernelGGL(k_lr_tsum, dim3(ntiles), dim3(256), 0, st, ws, nslab, ntiles, 0, k, cols, T + (int64_t)c0 * ldt, ldt);
  }
  return (int)hipGetLastError();
}

int chol_launch_lr_rprod(int64_t n, int k, int m, double alpha, double beta, const double *V, int64_t ldv, const double *T, int64_t ldt, double *X, int64_t ldx, hipStream_t st)
{
  if (n <= 0 || k <= 0 || m <= 0) return 0;
  if (k > CHOL_LR_MAX) return (int)hipErrorInvalidValue;
  const size_t lds = (size_t)((k + 3) & ~3) * CHOL_LR_ROWS * sizeof(double);
  const dim3 grid((unsigned)((n + CHOL_LR_ROWS - 1) / CHOL_LR_ROWS));
  if (m <= CHOL_NRHS_W) hipLaunchKernelGGL(k_lr_rprod32, grid, dim3(LRR_THREADS), lds, st, n, k, m, alpha, beta, V, ldv, T, ldt, X, ldx);
  else hipLaunchKernelGGL(k_lr_rprod, grid, dim3(LRR_THREADS), lds, st, n, k, m, alpha, beta, V, ldv, T, ldt, X, ldx);
  return (int)hipGetLastError();
}

int chol_launch_lr_rowsq(int64_t n, int k, const double *W, int64_t ldw, double *w, hipStream_t st)
{
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_lr_rowsq, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, k, W, ldw, w);
  return (int)hipGetLastError();
}

int chol_launch_lr_small(int what, int k, int cols, int mode, double *A, int64_t lda, const double *B, int64_t ldb, hipStream_t st)
{
  if (k <= 0 || cols <= 0) return 0;
  hipLaunchKernelGGL(k_lr_small, dim3((unsigned)((k * cols + 255) / 256)), dim3(256), 0, st, what, k, cols, mode, A, lda, B, ldb);
  return (int)hipGetLastError();
}
