// Selected inversion (cholamd_selinv): the entries of Z = (P A P^T)^-1 on the pattern of L, written into an arena of the factor's own layout.
//
// The Takahashi recursion over the separator tree, root first, in units of COLUMN BLOCKS J of at most CHOL_SELINV_W = 64 columns of a separator, last
// block first.  With "below" = the rows panel(s) stores after the block's last column (the separator's own rows, then the stored ancestor rows):
//   X       = L[J, J]^-1                                     k_selinv_inv     one workgroup per separator, substitution out of LDS
//   Y       = L[below, J] X                                  k_selinv_y       one wave per 16-row tile, 16 x 64 on v_mfma_f64_16x16x4_f64
//   Z[below, J] = -Z[below, below] Y                         k_selinv_gather  one wave per 16-row tile of the output; Z[below, below] is gathered tile
//                                                                             by tile through the row maps of the chain's panels (chol_selinv_level),
//                                                                             (i, j) or (j, i) of the stored lower triangle, 0.0 where nothing is stored
//   Z[J, J] = X^T X - Y^T Z[below, J]                        k_selinv_diag    one workgroup per 16 x 16 tile of the block's lower triangle, the rows
//                                                                             below split over four waves and summed in a fixed order
// All separators of one tree level are independent: step t of a level runs block nblk - 1 - t of every separator that has one (a prefix of the level's
// list), four launches per step, no waits between workgroups inside a launch.  Every output element has one owner and a fixed summation order; there is
// no floating-point atomic in this file, so two calls on one factor return the same bits.
// Y^T and Z[below, J]^T are kept row-major (64 doubles per panel row) in the workspace, so that the operand loads of the products are contiguous.
// MFMA operands as everywhere: lane l holds A(l & 15, k = l >> 4) and B(k = l >> 4, l & 15); result register q: row (l >> 4) + 4 q,
// column l & 15.
#include <hip/hip_runtime.h>

#include "chol_kernels.h"

typedef double nd4 __attribute__((ext_vector_type(4)));
#define SW CHOL_SELINV_W
#define SC (SW / 16)

struct sel_blk { int j0, j1, nb, t0; }; // columns [j0, j1) of the separator, nb of them; first tile of the rows below
__device__ __forceinline__ sel_blk sel_block(const chol_selinv_sep &d, int step)
{
  sel_blk b;
  b.j0 = (d.nblk - 1 - step) * SW;
  b.j1 = min(b.j0 + SW, d.w);
  b.nb = b.j1 - b.j0;
  b.t0 = b.j1 == d.w ? d.nown : b.j1 / CHOL_NB;
  return b;
}
__device__ __forceinline__ double *sel_yt(double *ws, const chol_selinv_sep &d) { return ws + d.ws_off; }
__device__ __forceinline__ double *sel_zt(double *ws, const chol_selinv_sep &d) { return ws + d.ws_off + (int64_t)d.prows * SW; }
__device__ __forceinline__ double *sel_x(double *ws, const chol_selinv_sep &d) { return ws + d.ws_off + 2 * (int64_t)d.prows * SW; }

// X = L[J, J]^-1 (lower triangular, zero outside nb x nb): thread c owns column c
__global__ __launch_bounds__(SW) void k_selinv_inv(const double *__restrict__ L, const chol_selinv_sep *__restrict__ seps, int step, double *__restrict__ ws)
{
  __shared__ double Ls[SW * SW], Xs[SW * SW]; // Ls[k * SW + i] = L(i, k); Xs[i * SW + c] = X(i, c)
  const chol_selinv_sep d = seps[blockIdx.x];
  const sel_blk b = sel_block(d, step);
  const int c = threadIdx.x;
  const double *A = L + d.panel_off + b.j0 + (int64_t)b.j0 * d.ld;
  for (int k = 0; k < SW; k++) Ls[k * SW + c] = (c < b.nb && k <= c) ? A[c + (int64_t)k * d.ld] : 0.0;
  __syncthreads();
  for (int i = 0; i < SW; i++) {
    double x = 0.0;
    if (c < b.nb && i < b.nb && i >= c) {
      double s = i == c ? 1.0 : 0.0;
      for (int k = c; k < i; k++) s -= Ls[k * SW + i] * Xs[k * SW + c];
      x = s / Ls[i * SW + i];
    }
    Xs[i * SW + c] = x;
  }
  __syncthreads();
  double *X = sel_x(ws, d); // row-major like Xs: the operand loads of k_selinv_y and k_selinv_diag read 16 consecutive doubles of a row
  for (int k = 0; k < SW; k++) X[k * SW + c] = Xs[k * SW + c];
}

// Y = L[below, J] X for one 16-row tile of the rows below
__global__ __launch_bounds__(64) void k_selinv_y(const double *__restrict__ L, const chol_selinv_sep *__restrict__ seps, const chol_selinv_tile *__restrict__ tiles, int step,
                                                 double *__restrict__ ws)
{
  const chol_selinv_sep d = seps[blockIdx.x];
  const sel_blk b = sel_block(d, step);
  const int ti = b.t0 + blockIdx.y;
  if (ti >= d.ntile) return;
  const chol_selinv_tile T = tiles[d.tile_first + ti];
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const double *Lp = L + d.panel_off + (int64_t)b.j0 * d.ld + T.q0;
  const double *X = sel_x(ws, d);
  nd4 acc[SC];
#pragma unroll
  for (int c = 0; c < SC; c++) acc[c] = (nd4){ 0.0, 0.0, 0.0, 0.0 };
  const bool rv = r < T.nrows;
  for (int k0 = 0; k0 < b.nb; k0 += 4) {
    const int k = k0 + g;
    const double a = rv && k < b.nb ? Lp[r + (int64_t)k * d.ld] : 0.0;
#pragma unroll
    for (int c = 0; c < SC; c++) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, X[k * SW + c * 16 + r], acc[c], 0, 0, 0);
  }
  double *Yt = sel_yt(ws, d);
#pragma unroll
  for (int c = 0; c < SC; c++)
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (g + 4 * q < T.nrows) Yt[(int64_t)(T.q0 + g + 4 * q) * SW + c * 16 + r] = acc[c][q];
}

// Z[below, J] = -Z[below, below] Y for one 16-row tile ti of the rows below: the sum over the tiles tj of the rows below in list order
__global__ __launch_bounds__(64) void k_selinv_gather(double *Z, const chol_selinv_sep *__restrict__ seps, const chol_selinv_tile *__restrict__ tiles,
                                                      const int *__restrict__ chain_ld, const int *__restrict__ chain_pos0, const int64_t *__restrict__ rowoff, int step,
                                                      double *__restrict__ ws)
{
  const chol_selinv_sep d = seps[blockIdx.x];
  const sel_blk b = sel_block(d, step);
  const int ti = b.t0 + blockIdx.y;
  if (ti >= d.ntile) return;
  const chol_selinv_tile *tl = tiles + d.tile_first;
  const chol_selinv_tile Ti = tl[ti];
  const int64_t *ro = rowoff + d.rowoff_first;
  const int *cld = chain_ld + d.chain_first, *cp0 = chain_pos0 + d.chain_first;
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const double *Yt = sel_yt(ws, d);
  nd4 acc[SC];
#pragma unroll
  for (int c = 0; c < SC; c++) acc[c] = (nd4){ 0.0, 0.0, 0.0, 0.0 };
  for (int tj = b.t0; tj < d.ntile; tj++) {
    const chol_selinv_tile Tj = tl[tj];
    // the stored (lower) side of tile pair (ti, tj): rows of the later tile, columns of the earlier one
    const chol_selinv_tile &Tc = tj <= ti ? Tj : Ti;
    const int64_t base = ro[(int64_t)(tj <= ti ? ti : tj) * d.nchain + Tc.k];
    if (base < 0) continue; // no storage: the block is structurally zero and reads as 0.0 (never an address from -1)
    const int ld = cld[Tc.k], col0 = Tc.pos0 - cp0[Tc.k];
    for (int k0 = 0; k0 < Tj.nrows; k0 += 4) {
      const int rj = k0 + g; // A(r, rj) = Z(row r of ti, row rj of tj)
      const bool kv = rj < Tj.nrows;
      double a = 0.0;
      if (kv && r < Ti.nrows) {
        int hi, lo;
        if (tj < ti) { hi = r; lo = rj; } else if (tj > ti) { hi = rj; lo = r; } else { hi = max(r, rj); lo = min(r, rj); }
        a = Z[base + hi + (int64_t)(col0 + lo) * ld];
      }
      const double *yr = Yt + (int64_t)(Tj.q0 + rj) * SW + r;
#pragma unroll
      for (int c = 0; c < SC; c++) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, kv ? yr[c * 16] : 0.0, acc[c], 0, 0, 0);
    }
  }
  double *Zt = sel_zt(ws, d);
  double *Zp = Z + d.panel_off + (int64_t)b.j0 * d.ld + Ti.q0;
#pragma unroll
  for (int c = 0; c < SC; c++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int row = g + 4 * q, col = c * 16 + r;
      if (row < Ti.nrows) {
        const double v = -acc[c][q];
        Zt[(int64_t)(Ti.q0 + row) * SW + col] = v;
        if (col < b.nb) Zp[row + (int64_t)col * d.ld] = v;
      }
    }
}

// Z[J, J] = X^T X - Y^T Z[below, J], one 16 x 16 tile (ta, tb), ta >= tb, of the block's lower triangle per workgroup
__global__ __launch_bounds__(256) void k_selinv_diag(double *__restrict__ Z, const chol_selinv_sep *__restrict__ seps, int step, const double *__restrict__ ws_c)
{
  __shared__ double red[4][256];
  double *ws = const_cast<double *>(ws_c);
  const chol_selinv_sep d = seps[blockIdx.x];
  const sel_blk b = sel_block(d, step);
  int ta, tb;
  chol_rr_tile_of_index(blockIdx.y, SC, &ta, &tb);
  if (ta * 16 >= b.nb) return; // (the whole workgroup)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const double *Yt = sel_yt(ws, d), *Zt = sel_zt(ws, d), *X = sel_x(ws, d);
  const int m = d.prows - b.j1, per = ((m + 15) / 16) * 4; // rows below, rows per wave (a multiple of four)
  const int lo = b.j1 + wv * per, hi = min(d.prows, lo + per);
  nd4 acc = (nd4){ 0.0, 0.0, 0.0, 0.0 };
  for (int q0 = lo; q0 < hi; q0 += 4) {
    const int q = q0 + g;
    const bool ok = q < hi;
    const double av = ok ? Yt[(int64_t)q * SW + ta * 16 + r] : 0.0, bv = ok ? Zt[(int64_t)q * SW + tb * 16 + r] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
  }
#pragma unroll
  for (int q = 0; q < 4; q++) red[wv][q * 64 + lane] = acc[q];
  __syncthreads();
  if (wv != 0) return;
  nd4 xx = (nd4){ 0.0, 0.0, 0.0, 0.0 };
  for (int k0 = 0; k0 < b.nb; k0 += 4) {
    const int k = k0 + g;
    xx = __builtin_amdgcn_mfma_f64_16x16x4f64(X[k * SW + ta * 16 + r], X[k * SW + tb * 16 + r], xx, 0, 0, 0);
  }
  double *Zp = Z + d.panel_off + b.j0 + (int64_t)b.j0 * d.ld;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const double s = ((red[0][q * 64 + lane] + red[1][q * 64 + lane]) + red[2][q * 64 + lane]) + red[3][q * 64 + lane]; // the waves' partial sums in a fixed order
    const int row = ta * 16 + g + 4 * q, col = tb * 16 + r;
    if (row < b.nb && col < b.nb && row >= col) Zp[row + (int64_t)col * d.ld] = xx[q] - s;
  }
}

// entries of A^-1 in value-array order: NaN everywhere, then entry a_src[e] of the scatter list from the arena position the scatter writes it to
__global__ void k_selinv_entries_nan(double *__restrict__ vals, int64_t nz)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nz) vals[i] = __longlong_as_double(0x7ff8000000000000LL);
}
__global__ void k_selinv_entries(const double *__restrict__ Z, const int64_t *__restrict__ a_dst, const int *__restrict__ a_src, int64_t nnz, double *__restrict__ vals)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < nnz) vals[a_src[e]] = Z[a_dst[e]];
}

// the separators of a step lie on grid.x (a deep tree level has more of them than grid.y takes), the tiles below on grid.y (CHOL_SELINV_MAX_TILES)
int chol_launch_selinv_step(const double *L, double *Z, double *ws, const chol_selinv_sep *seps, int n_act, const chol_selinv_tile *tiles, const int *chain_ld,
                            const int *chain_pos0, const int64_t *rowoff, int step, int max_below_tiles, hipStream_t st)
{
  if (n_act <= 0) return 0;
  if (max_below_tiles > CHOL_SELINV_MAX_TILES) return (int)hipErrorInvalidConfiguration;
  hipError_t e;
  hipLaunchKernelGGL(k_selinv_inv, dim3(n_act), dim3(SW), 0, st, L, seps, step, ws);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if (max_below_tiles > 0) {
    hipLaunchKernelGGL(k_selinv_y, dim3(n_act, max_below_tiles), dim3(64), 0, st, L, seps, tiles, step, ws);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_selinv_gather, dim3(n_act, max_below_tiles), dim3(64), 0, st, Z, seps, tiles, chain_ld, chain_pos0, rowoff, step, ws);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(k_selinv_diag, dim3(n_act, SC * (SC + 1) / 2), dim3(256), 0, st, Z, seps, step, (const double *)ws);
  return (int)hipGetLastError();
}
int chol_launch_selinv_entries(const double *Z, const int64_t *a_dst, const int *a_src, int64_t nnz, double *vals, int64_t nz, hipStream_t st)
{
  if (nz > 0) {
    hipLaunchKernelGGL(k_selinv_entries_nan, dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, st, vals, nz);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  if (nnz > 0) hipLaunchKernelGGL(k_selinv_entries, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, Z, a_dst, a_src, nnz, vals);
  return (int)hipGetLastError();
}
