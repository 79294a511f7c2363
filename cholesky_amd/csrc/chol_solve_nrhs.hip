// Block solve: many right-hand sides per pass over the factor (cholamd_solve_nrhs / _f32 / cholamd_solve_refine_nrhs).
//
// The right-hand sides are solved in chunks of CHOL_NRHS_W = 32 columns.  A chunk lives in the permuted block Y (n x 32, ROW-major: the 32 values of one
// permuted row are 256 contiguous bytes) and gets one forward and one backward sweep over the solve lists of the single-vector path (chol_solve_level:
// the separators' diagonal blocks, the row runs `bw` of their (ancestor, separator) blocks cut into the `ifw` / `ibw` work items), so every stored entry of
// L is read once per sweep per chunk and carries 64 flops instead of 2.  Every product is a tile of 16 rows x 32 right-hand sides on
// v_mfma_f64_16x16x4_f64 (two accumulators per wave): the off-diagonal blocks, the rows of a wide separator under a 256-column span, the 16x16 diagonal
// inverses of the substitution chain and the explicit 256-column span inverses where the solve lists have them.  The factor's element type TL is double
// or float (the fp32 factor of the mixed-precision path: converted on load); vectors and arithmetic are fp64.
//
// Launch structure per level (no waits between workgroups inside a launch):
//   forward:  per 256-column span: k_nrhs_span (one workgroup per separator: the span's triangle, out of LDS) then k_nrhs_panel (the rows under the span
//             over all CUs); then k_nrhs_offdiag (the ifw items: Y_anc -= L(rows, sep) X_sep, fp64 atomics into Y)
//   backward: k_nrhs_offdiag (the ibw items: X_sep -= L(rows, sep)^T Y_anc), then per span in reverse: k_nrhs_panel (gather), k_nrhs_span (transposed)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chol_kernels.h"
#include "chol_plan.h"

#define NW CHOL_NRHS_W   // right-hand sides per chunk: two 16-column MFMA tiles
#define NSPAN 256        // span of the diagonal solve (= SSPAN of chol_solve.hip, the span of the explicit inverses)
#define NT 16            // MFMA tile
#define NPANEL_ROWS 256  // rows under a span per workgroup of k_nrhs_panel
static_assert(NW == 32, "Y rows are two 16-column tiles");

typedef double nd4 __attribute__((ext_vector_type(4)));

// Position of element (r, c) of a block with NW columns: row-major (SW = false: Y in global memory) or, in LDS (SW = true), with the two 16-column halves
// of every odd row swapped.  A B-operand read (ds_read_b64, lane groups {0-31}, {32-63}, bank = dword mod 64) has rows k and k + 1 in one lane group; at a
// 256-byte row pitch both rows' 16 doubles fall on the same 32 banks (2-way conflict), swapped they take the other half of the banks.  Tiles start at even
// rows, so the swizzle relative to a tile's first row is the block's own.
template <bool SW> __device__ __forceinline__ int64_t bpos(int64_t r, int c) { return r * NW + (SW ? (c ^ (((int)r & 1) << 4)) : c); }

// acc(i, j) += sum_{k < kv} op(L)(i, k) B(k, j) for the 16 rows i of a tile and the 32 columns j of the chunk, one wave.
//   op(L)(i, k) = L[i + k * lda] (TR = false) or L[k + i * lda] (TR = true); rows i >= mv are read clamped (their results are not stored)
//   B: NW columns, element (k, j) at bpos<SW>(k, j) (a part of Y, or of LDS)
// MFMA operands (v_mfma_f64_16x16x4_f64): lane l holds A(l & 15, k = l >> 4) and B(k = l >> 4, l & 15); result register q: row (l >> 4) + 4 q, column l & 15.
template <bool TR, bool SW = false, class TL>
__device__ __forceinline__ void tile_mm(const TL *__restrict__ L, int lda, int mv, int kv, const double *B, nd4 &acc0, nd4 &acc1)
{
  const int lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
  const int i = min(i16, mv - 1);
  constexpr int U = 8; // k-steps of four whose loads are in flight together
  for (int k0 = 0; k0 < kv; k0 += 4 * U) {
    double a[U], b0[U], b1[U];
#pragma unroll
    for (int s = 0; s < U; ++s) {
      const int k = k0 + 4 * s + g, kk = min(k, kv - 1);
      const double v = TR ? (double)L[kk + (int64_t)i * lda] : (double)L[i + (int64_t)kk * lda];
      a[s] = k < kv ? v : 0.0;
      b0[s] = B[bpos<SW>(kk, i16)];
      b1[s] = B[bpos<SW>(kk, 16 + i16)];
    }
#pragma unroll
    for (int s = 0; s < U; ++s) {
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b0[s], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b1[s], acc1, 0, 0, 0);
    }
  }
}
// Y(r, j) -= acc(r, j) for the rows r < mv of a tile (Y: row-major, its first row); ATOMIC: other workgroups add to the same rows
template <bool ATOMIC, bool SW = false>
__device__ __forceinline__ void tile_sub(double *Y, int mv, const nd4 &acc0, const nd4 &acc1)
{
  const int lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = g + 4 * q;
    if (r < mv) {
      if (ATOMIC) {
        unsafeAtomicAdd(&Y[bpos<SW>(r, i16)], -acc0[q]);
        unsafeAtomicAdd(&Y[bpos<SW>(r, 16 + i16)], -acc1[q]);
      } else {
        Y[bpos<SW>(r, i16)] -= acc0[q];
        Y[bpos<SW>(r, 16 + i16)] -= acc1[q];
      }
    }
  }
}
__device__ __forceinline__ void tile_put(double *Y, int mv, const nd4 &acc0, const nd4 &acc1) // (LDS: swizzled)
{
  const int lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = g + 4 * q;
    if (r < mv) { Y[bpos<true>(r, i16)] = acc0[q]; Y[bpos<true>(r, 16 + i16)] = acc1[q]; }
  }
}

// Y[i][j] = B[perm[i] + (c0 + j) ldb] for the chunk's columns j < cols, 0 past them (the padding columns stay zero through the sweeps)
__global__ __launch_bounds__(256) void k_nrhs_permute_in(const double *__restrict__ B, int64_t ldb, const int *__restrict__ perm, double *__restrict__ Y, int n, int c0, int cols)
{
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n * NW) return;
  const int i = (int)(e / NW), j = (int)(e % NW);
  Y[e] = j < cols ? B[perm[i] + (int64_t)(c0 + j) * ldb] : 0.0;
}
__global__ __launch_bounds__(256) void k_nrhs_permute_out(const double *__restrict__ Y, const int *__restrict__ perm, double *__restrict__ X, int64_t ldx, int n, int c0, int cols)
{
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n * NW) return;
  const int i = (int)(e / NW), j = (int)(e % NW);
  if (j < cols) X[perm[i] + (int64_t)(c0 + j) * ldx] = Y[e];
}

// The diagonal triangle of one 256-column span [col0, col0 + 256) of every separator of a level (one workgroup each) on the chunk's 32 columns; the span's
// rows of Y stay in LDS (swizzled: bpos).  With the span's explicit inverse W (k_solve_inv256: [column][row], 16x16 blocks on and below the diagonal) X = W R (forward) /
// W^T R (backward) is one product with no chain.  Without: sixteen 16-column block steps, X_j = Dinv_j R_j (Dinv_j^T R_j) on wave 0, then every wave folds
// X_j into its tiles of the span's other rows (forward: below, backward: in front).
template <bool BWD, class TL>
__global__ __launch_bounds__(256) void k_nrhs_span(const TL *__restrict__ base, const chol_trsv_desc *__restrict__ descs, const double *__restrict__ W16all,
                                                   const double *__restrict__ W256, int nspan_max, double *__restrict__ Y, int col0)
{
  __shared__ double sY[NSPAN * NW];
  const chol_trsv_desc d = descs[blockIdx.x];
  if (d.n <= col0) return;
  const int ns = min(d.n - col0, NSPAN), nb = (ns + NT - 1) / NT, wave = threadIdx.x >> 6;
  double *Yg = Y + (int64_t)(d.x_off + col0) * NW;
  for (int e = threadIdx.x; e < NSPAN * NW; e += 256) sY[bpos<true>(e / NW, e % NW)] = e < ns * NW ? Yg[e] : 0.0;
  __syncthreads();
  const TL *Lm = base + d.a_off + col0 + (int64_t)col0 * d.lda;
  const double *W16 = W16all + d.dinv_off + (int64_t)(col0 / NT) * NT * NT; // block b: W16[b * 256 + c * 16 + r] = inv(L_bb)(r, c)
  if (W256) {
    const double *Ws = W256 + ((int64_t)blockIdx.x * nspan_max + col0 / NSPAN) * (NSPAN * NSPAN);
    nd4 acc[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      acc[t][0] = (nd4){ 0.0, 0.0, 0.0, 0.0 };
      acc[t][1] = (nd4){ 0.0, 0.0, 0.0, 0.0 };
      const int i = wave + 4 * t;
      if (i >= nb) continue;
      if (!BWD) { // X_i = sum_{k <= i} W(i, k) R_k
        tile_mm<false, true>(Ws + NT * i, NSPAN, NT, min(NT * (i + 1), ns), sY, acc[t][0], acc[t][1]);
      } else {    // X_i = sum_{k >= i} W(k, i)^T R_k
        tile_mm<true, true>(Ws + NT * i + (int64_t)(NT * i) * NSPAN, NSPAN, NT, ns - NT * i, sY + NT * i * NW, acc[t][0], acc[t][1]);
      }
    }
    __syncthreads(); // every wave has read R
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int i = wave + 4 * t;
      if (i < nb) tile_put(sY + NT * i * NW, min(NT, ns - NT * i), acc[t][0], acc[t][1]);
    }
  } else {
    for (int s = 0; s < nb; ++s) {
      const int j = BWD ? nb - 1 - s : s, mj = min(NT, ns - NT * j);
      if (wave == 0) {
        nd4 a0 = { 0.0, 0.0, 0.0, 0.0 }, a1 = { 0.0, 0.0, 0.0, 0.0 };
        tile_mm<BWD, true>(W16 + j * NT * NT, NT, NT, NT, sY + NT * j * NW, a0, a1); // (W16 has identity padding past n; R rows past ns are zero)
        tile_put(sY + NT * j * NW, mj, a0, a1);
      }
      __syncthreads();
      // forward: tiles t > j, sY_t -= L(t, j) X_j; backward: tiles t < j, sY_t -= L(j, t)^T X_j
      const int t0 = BWD ? 0 : j + 1, t1 = BWD ? j : nb;
      for (int t = t0 + wave; t < t1; t += 4) {
        nd4 a0 = { 0.0, 0.0, 0.0, 0.0 }, a1 = { 0.0, 0.0, 0.0, 0.0 };
        const int mt = min(NT, ns - NT * t);
        if (!BWD) tile_mm<false, true>(Lm + NT * t + (int64_t)(NT * j) * d.lda, d.lda, mt, mj, sY + NT * j * NW, a0, a1);
        else tile_mm<true, true>(Lm + NT * j + (int64_t)(NT * t) * d.lda, d.lda, mt, mj, sY + NT * j * NW, a0, a1);
        tile_sub<false, true>(sY + NT * t * NW, mt, a0, a1);
      }
      __syncthreads();
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < ns * NW; e += 256) Yg[e] = sY[bpos<true>(e / NW, e % NW)];
}

// The rows of a separator under the span [col0, col0 + 256) (a leaf's band bounds them), NPANEL_ROWS per workgroup, four row tiles (forward) / the span's
// sixteen column tiles (backward) per wave.  Forward: Y(rows) -= L(rows, span) X_span (the rows are the workgroup's own); backward: X_span -= L(rows, span)^T
// Y(rows) (fp64 atomics: every row chunk adds to the same span)
template <bool BWD, class TL>
__global__ __launch_bounds__(256) void k_nrhs_panel(const TL *__restrict__ base, const chol_trsv_desc *__restrict__ descs, double *__restrict__ Y, int col0)
{
  const chol_trsv_desc d = descs[blockIdx.x];
  const int r0 = col0 + NSPAN;
  const int n = d.band > 0 ? min(d.n, r0 + d.band) : d.n;
  const int row0 = r0 + (int)blockIdx.y * NPANEL_ROWS;
  if (n <= row0) return;
  const int rows = min(n - row0, NPANEL_ROWS), wave = threadIdx.x >> 6;
  const TL *Lm = base + d.a_off;
  double *Ys = Y + (int64_t)(d.x_off + col0) * NW, *Yr = Y + (int64_t)(d.x_off + row0) * NW;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int t = wave + 4 * u;
    nd4 a0 = { 0.0, 0.0, 0.0, 0.0 }, a1 = { 0.0, 0.0, 0.0, 0.0 };
    if (!BWD) {
      if (NT * t >= rows) break;
      tile_mm<false>(Lm + row0 + NT * t + (int64_t)col0 * d.lda, d.lda, min(NT, rows - NT * t), NSPAN, Ys, a0, a1);
      tile_sub<false>(Yr + NT * t * NW, min(NT, rows - NT * t), a0, a1);
    } else {
      const int ns = min(d.n - col0, NSPAN);
      if (NT * t >= ns) break;
      tile_mm<true>(Lm + row0 + (int64_t)(col0 + NT * t) * d.lda, d.lda, min(NT, ns - NT * t), rows, Yr, a0, a1);
      tile_sub<true>(Ys + NT * t * NW, min(NT, ns - NT * t), a0, a1);
    }
  }
}

// The (ancestor, separator) blocks of a level.  Forward (ifw items: block run, first row, first column, first non-zero column): rows [r, r + 256) of the run
// x columns [c, c + 1024), four row tiles per wave, Y_anc -= L X_sep by fp64 atomics (other column chunks and other separators add to the same rows).
// Backward (ibw items: first run, end run, first column, 0): sixteen columns of ONE separator per wave over the runs [q0, q1), X_sep -= L^T Y_anc, one atomic
// per element per workgroup.
template <bool BWD, class TL>
__global__ __launch_bounds__(256) void k_nrhs_offdiag(const TL *__restrict__ base, const chol_gemv_desc *__restrict__ blocks, const int *__restrict__ items, double *__restrict__ Y)
{
  const int *it = items + 4 * blockIdx.x;
  const int wave = threadIdx.x >> 6;
  if (!BWD) {
    const chol_gemv_desc d = blocks[it[0]];
    const int r0 = it[1], c0 = max(it[2], it[3]), c1 = min(d.n, it[2] + CHOL_SOLVE_COLS);
    if (c0 >= c1) return;
    const int rows = min(d.m - r0, CHOL_SOLVE_FW_ROWS);
#pragma unroll
    for (int u = 0; u < CHOL_SOLVE_FW_ROWS / NT / 4; ++u) {
      const int t = wave + 4 * u;
      if (NT * t >= rows) break;
      nd4 a0 = { 0.0, 0.0, 0.0, 0.0 }, a1 = { 0.0, 0.0, 0.0, 0.0 };
      const int mt = min(NT, rows - NT * t);
      tile_mm<false>(base + d.a_off + r0 + NT * t + (int64_t)c0 * d.lda, d.lda, mt, c1 - c0, Y + (int64_t)(d.y_off + c0) * NW, a0, a1);
      tile_sub<true>(Y + (int64_t)(d.x_off + r0 + NT * t) * NW, mt, a0, a1);
    }
  } else {
    const int q0 = it[0], q1 = it[1];
    const int n = blocks[q0].n, cw = it[2] + NT * wave;
    if (cw >= n) return;
    const int nc = min(NT, n - cw);
    nd4 a0 = { 0.0, 0.0, 0.0, 0.0 }, a1 = { 0.0, 0.0, 0.0, 0.0 };
    for (int b = q0; b < q1; ++b) {
      const chol_gemv_desc d = blocks[b];
      if (d.c_lo >= cw + NT || d.m <= 0) continue; // the run's rows are zero in these columns
      tile_mm<true>(base + d.a_off + (int64_t)cw * d.lda, d.lda, nc, d.m, Y + (int64_t)d.x_off * NW, a0, a1);
    }
    tile_sub<true>(Y + (int64_t)(blocks[q0].y_off + cw) * NW, nc, a0, a1);
  }
}

// Refinement: R(:, j) = B(:, j) - A X(:, j) for the chunk's columns (A: both triangles, CSR in original dof order), per-workgroup partial sums of r_j^2 and
// b_j^2 (summed on the host: deterministic); grid (row blocks, columns)
__global__ __launch_bounds__(256) void k_nrhs_residual(const int64_t *__restrict__ ptr, const int *__restrict__ col, const double *__restrict__ val,
                                                       const double *__restrict__ B, int64_t ldb, const double *__restrict__ X, int64_t ldx,
                                                       double *__restrict__ R, int64_t ldr, int n, double *__restrict__ partial)
{
  __shared__ double s2[2][4];
  const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  const double *b = B + (int64_t)j * ldb, *x = X + (int64_t)j * ldx;
  double ri = 0.0, bi = 0.0;
  if (i < n) {
    bi = b[i];
    double acc = bi;
    for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) acc = fma(-val[e], x[col[e]], acc);
    ri = acc;
    R[i + (int64_t)j * ldr] = ri;
  }
  double a = ri * ri, c = bi * bi;
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); c += __shfl_down(c, o, 64); }
  if ((threadIdx.x & 63) == 0) { s2[0][threadIdx.x >> 6] = a; s2[1][threadIdx.x >> 6] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double *p = partial + 2 * ((int64_t)j * gridDim.x + blockIdx.x);
    p[0] = ((s2[0][0] + s2[0][1]) + s2[0][2]) + s2[0][3];
    p[1] = ((s2[1][0] + s2[1][1]) + s2[1][2]) + s2[1][3];
  }
}
// X(:, j) += D(:, j), grid (row blocks, columns)
__global__ __launch_bounds__(256) void k_nrhs_axpy(double *__restrict__ X, int64_t ldx, const double *__restrict__ D, int64_t ldd, int n)
{
  const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  if (i < n) X[i + (int64_t)j * ldx] += D[i + (int64_t)j * ldd];
}

template <class TL>
int chol_nrhs_launch_trsv(const TL *base, const chol_trsv_desc *descs, int n, int max_n, int max_under, const double *W16, const double *W256, double *Y, int backward, hipStream_t st)
{
  if (n <= 0 || max_n <= 0) return 0;
  const int nspan = (max_n + NSPAN - 1) / NSPAN, mu = max_under < 0 ? -max_under : max_under;
  for (int i = 0; i < nspan; i++) {
    const int sp = backward ? nspan - 1 - i : i, col0 = sp * NSPAN;
    const int below = min(max_n - (col0 + NSPAN), mu); // rows under the span in the widest separator
    const dim3 pgrid(n, below > 0 ? (below + NPANEL_ROWS - 1) / NPANEL_ROWS : 1);
    if (backward) {
      if (below > 0) hipLaunchKernelGGL((k_nrhs_panel<true, TL>), pgrid, dim3(256), 0, st, base, descs, Y, col0);
      hipLaunchKernelGGL((k_nrhs_span<true, TL>), dim3(n), dim3(256), 0, st, base, descs, W16, W256, nspan, Y, col0);
    } else {
      hipLaunchKernelGGL((k_nrhs_span<false, TL>), dim3(n), dim3(256), 0, st, base, descs, W16, W256, nspan, Y, col0);
      if (below > 0) hipLaunchKernelGGL((k_nrhs_panel<false, TL>), pgrid, dim3(256), 0, st, base, descs, Y, col0);
    }
  }
  return (int)hipGetLastError();
}
// The span [col0, col0 + 256) of every separator of `descs` by the substitution chain of the 16x16 inverses (W256 = NULL), and nothing else: the span
// step of the deterministic block solve (option solve_deterministic_block), whose rows outside the span are the business of its gather launches.
template <class TL> int chol_nrhs_launch_span(const TL *base, const chol_trsv_desc *descs, int n_descs, const double *W16, double *Y, int col0, int backward, hipStream_t st)
{
  if (n_descs <= 0) return 0;
  if (backward) hipLaunchKernelGGL((k_nrhs_span<true, TL>), dim3(n_descs), dim3(256), 0, st, base, descs, W16, (const double *)nullptr, 0, Y, col0);
  else hipLaunchKernelGGL((k_nrhs_span<false, TL>), dim3(n_descs), dim3(256), 0, st, base, descs, W16, (const double *)nullptr, 0, Y, col0);
  return (int)hipGetLastError();
}
template <class TL> int chol_nrhs_launch_offdiag(const TL *base, const chol_gemv_desc *blocks, const int *items, int n_items, double *Y, int backward, hipStream_t st)
{
  if (n_items <= 0) return 0;
  if (backward) hipLaunchKernelGGL((k_nrhs_offdiag<true, TL>), dim3(n_items), dim3(256), 0, st, base, blocks, items, Y);
  else hipLaunchKernelGGL((k_nrhs_offdiag<false, TL>), dim3(n_items), dim3(256), 0, st, base, blocks, items, Y);
  return (int)hipGetLastError();
}

int chol_nrhs_launch_permute(const double *B, int64_t ldb, const int *perm, double *Y, double *X, int64_t ldx, int n, int c0, int cols, int inverse, hipStream_t st)
{
  if (n <= 0) return 0;
  const unsigned blocks = (unsigned)(((int64_t)n * NW + 255) / 256);
  if (inverse) hipLaunchKernelGGL(k_nrhs_permute_out, dim3(blocks), dim3(256), 0, st, Y, perm, X, ldx, n, c0, cols);
  else hipLaunchKernelGGL(k_nrhs_permute_in, dim3(blocks), dim3(256), 0, st, B, ldb, perm, Y, n, c0, cols);
  return (int)hipGetLastError();
}
template int chol_nrhs_launch_trsv(const double *, const chol_trsv_desc *, int, int, int, const double *, const double *, double *, int, hipStream_t);
template int chol_nrhs_launch_trsv(const float *, const chol_trsv_desc *, int, int, int, const double *, const double *, double *, int, hipStream_t);
template int chol_nrhs_launch_span(const double *, const chol_trsv_desc *, int, const double *, double *, int, int, hipStream_t);
template int chol_nrhs_launch_span(const float *, const chol_trsv_desc *, int, const double *, double *, int, int, hipStream_t);
template int chol_nrhs_launch_offdiag(const double *, const chol_gemv_desc *, const int *, int, double *, int, hipStream_t);
template int chol_nrhs_launch_offdiag(const float *, const chol_gemv_desc *, const int *, int, double *, int, hipStream_t);
int chol_nrhs_launch_residual(const int64_t *ptr, const int *col, const double *val, const double *B, int64_t ldb, const double *X, int64_t ldx, double *R, int64_t ldr,
                              int n, int cols, double *partial, hipStream_t st)
{
  if (n <= 0 || cols <= 0) return 0;
  hipLaunchKernelGGL(k_nrhs_residual, dim3((n + 255) / 256, cols), dim3(256), 0, st, ptr, col, val, B, ldb, X, ldx, R, ldr, n, partial);
  return (int)hipGetLastError();
}
int chol_nrhs_launch_axpy(double *X, int64_t ldx, const double *D, int64_t ldd, int n, int cols, hipStream_t st)
{
  if (n <= 0 || cols <= 0) return 0;
  hipLaunchKernelGGL(k_nrhs_axpy, dim3((n + 255) / 256, cols), dim3(256), 0, st, X, ldx, D, ldd, n);
  return (int)hipGetLastError();
}
