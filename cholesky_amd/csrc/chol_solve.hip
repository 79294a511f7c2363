// HIP kernels of libcholamd for gfx950 (MI355X, CDNA4): the streamed triangular solve on the fp64 and the fp32 factor (permutation, the
// level kernels of the forward and backward sweeps, the span / step / leaf kernels and their launchers) and the helpers of the fp64
// iterative refinement.  Descriptors, offsets and MFMA operand maps as in chol_kernels.hip.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "chol_plan.h"
#include "chol_kernels.h"
#include "chol_wave.h"

#define NB 32 /* block width of the triangular solves below */
// ------------------------------------------------------------------------------------------------
// Solve phase (mmat.rg:1364-1495).  Vectors live in permuted order.
// ------------------------------------------------------------------------------------------------
__global__ void k_permute_in(const double *__restrict__ b, const int *__restrict__ perm, double *__restrict__ y, int n)
{ // fill_b, mmat.rg:769-783: y[pos] = b[perm[pos]]
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = b[perm[i]];
}
__global__ void k_permute_out(const double *__restrict__ y, const int *__restrict__ perm, double *__restrict__ x, int n)
{ // mmat.rg:1483-1491: x[perm[pos]] = y[pos]
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[perm[i]] = y[i];
}

// forward level step: for each separator s of the level (one workgroup each):
//   y_s <- L_ss^-1 y_s (cblas_dtrsv Lower/NoTrans, blas.rg:226), blocked by 32 with the panel GEMV
__global__ __launch_bounds__(256) void k_trsv_fwd(const double *__restrict__ base, const chol_trsv_desc *__restrict__ descs, double *__restrict__ y)
{
  __shared__ double sx[32];
  const chol_trsv_desc d = descs[blockIdx.x];
  const double *Lm = base + d.a_off;
  double *x = y + d.x_off;
  const int n = d.n, lda = d.lda, tid = threadIdx.x;
  for (int j0 = 0; j0 < n; j0 += NB) {
    const int jb = min(NB, n - j0);
    if (tid < 64) { // one wave solves the 32x32 triangle, lane = row
      const int r = tid & 31;
      double v = (tid < jb) ? x[j0 + r] : 0.0;
      for (int j = 0; j < jb; ++j) {
        const double dj = Lm[(j0 + j) + (int64_t)(j0 + j) * lda];
        const double xj = __shfl(v, j, 64) / dj;
        if (r == j) v = xj;
        else if (r > j && r < jb) v -= xj * Lm[(j0 + r) + (int64_t)(j0 + j) * lda];
      }
      if (tid < jb) { x[j0 + r] = v; sx[r] = v; }
    }
    __syncthreads();
    for (int rr = j0 + jb + tid; rr < n; rr += 256) {
      double acc = 0.0;
      for (int k = 0; k < jb; ++k) acc += Lm[rr + (int64_t)(j0 + k) * lda] * sx[k];
      x[rr] -= acc;
    }
    __syncthreads();
  }
}

// y_t <- y_t - sum over sources A x   (cblas_dgemv NoTrans alpha=-1 beta=1, blas.rg:263), target-
// centric: one workgroup per 256 rows of a target separator, sources in program order.
__global__ __launch_bounds__(256) void k_gemv_fwd(const double *__restrict__ base, const chol_gemv_desc *__restrict__ descs,
                                                  const int *__restrict__ grp_start, const int *__restrict__ grp_rows, double *__restrict__ y)
{
  const int g = blockIdx.x;
  const int row0 = grp_rows[2 * g], y_off = grp_rows[2 * g + 1];
  const int r = row0 + threadIdx.x;
  double acc = 0.0;
  bool valid = false;
  for (int s = grp_start[g]; s < grp_start[g + 1]; ++s) {
    const chol_gemv_desc d = descs[s];
    const int rr = r - d.y_off; // the source's rows start at row y_off of the target separator (a stored row run of its block)
    if (rr >= 0 && rr < d.m) {
      valid = true;
      const double *A = base + d.a_off + rr;
      const double *x = y + d.x_off;
      for (int k = 0; k < d.n; ++k) acc += A[(int64_t)k * d.lda] * x[k];
    }
  }
  if (valid) y[y_off + r] -= acc;
}

// backward level step for separator s: y_s <- y_s - sum_anc A(anc,s)^T y_anc  (cblas_dgemv Trans),
// then y_s <- L_ss^-T y_s (cblas_dtrsv Lower/Trans).  One workgroup per separator.
__global__ __launch_bounds__(256) void k_bwd(const double *__restrict__ base, const chol_trsv_desc *__restrict__ descs,
                                             const chol_gemv_desc *__restrict__ gd, const int *__restrict__ gstart, double *__restrict__ y)
{
  __shared__ double sx[32];
  __shared__ double red[256];
  const chol_trsv_desc d = descs[blockIdx.x];
  const double *Lm = base + d.a_off;
  double *x = y + d.x_off;
  const int n = d.n, lda = d.lda, tid = threadIdx.x;
  // gather from ancestors: column c of A^T x = dot(A[:, c], x_anc)
  for (int s = gstart[blockIdx.x]; s < gstart[blockIdx.x + 1]; ++s) {
    const chol_gemv_desc g = gd[s];
    const double *A = base + g.a_off;
    const double *xa = y + g.x_off;
    for (int c0 = 0; c0 < g.n; c0 += 4) { // 4 columns at a time, 64 threads per column
      const int c = c0 + (tid >> 6), l = tid & 63;
      double acc = 0.0;
      if (c < g.n)
        for (int i = l; i < g.m; i += 64) acc += A[i + (int64_t)c * g.lda] * xa[i];
      for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
      if (l == 0 && c < g.n) x[c] -= acc;
    }
    __syncthreads();
  }
  // L^T x = b, blocks from the bottom up
  const int nblk = (n + NB - 1) / NB;
  for (int jb_i = nblk - 1; jb_i >= 0; --jb_i) {
    const int j0 = jb_i * NB, jb = min(NB, n - j0);
    // x_J -= L[J+1.., J]^T x_{J+1..}: column c of the panel dotted with the solved tail
    {
      const int c = tid >> 3, l = tid & 7; // 32 columns x 8 threads
      double acc = 0.0;
      if (c < jb)
        for (int i = j0 + jb + l; i < n; i += 8) acc += Lm[i + (int64_t)(j0 + c) * lda] * x[i];
      red[tid] = acc;
      __syncthreads();
      if (tid < NB) {
        double s = 0.0;
        for (int q = 0; q < 8; ++q) s += red[tid * 8 + q];
        sx[tid] = (tid < jb) ? x[j0 + tid] - s : 0.0;
      }
      __syncthreads();
    }
    if (tid < 64) { // triangle solve, lane = column index, backwards
      const int r = tid & 31;
      double v = (r < jb) ? sx[r] : 0.0;
      for (int j = jb - 1; j >= 0; --j) {
        const double dj = Lm[(j0 + j) + (int64_t)(j0 + j) * lda];
        const double xj = __shfl(v, j, 64) / dj;
        if (r == j) v = xj;
        else if (r < j) v -= xj * Lm[(j0 + j) + (int64_t)(j0 + r) * lda];
      }
      if (tid < jb) x[j0 + r] = v;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// Driver-level solve (cholamd_solve) at scale.  The kernels above keep the reference's per-call shape (one
// workgroup per separator / per 256 target rows, dependent loads per column) and serve the BLAS-level entry
// points; on a 10^6-unknown factor they take seconds.  These stream every panel once instead:
//   * diagonal blocks: the 16x16 inverses of all diagonal blocks are recomputed into the solve workspace
//     (k_solve_dinv: the factorisation's workspace belongs to the last arena factored, not to this one), and
//     the triangular solves run in 64-column block steps with the in-block work done out of LDS
//   * off-diagonal blocks: one workgroup per row chunk of an (ancestor, separator) block, source-centric,
//     accumulating into y with hardware fp64 atomics (the only non-deterministic summation order in the library:
//     the solution agrees from run to run to rounding, not bit for bit; option solve_deterministic replaces these kernels by the
//     owner gathers of chol_solve_det.hip and keeps only the span solvers of this file)
// ------------------------------------------------------------------------------------------------
#define SNB 64
// The driver-level solve kernels are templates over the factor's element type TL (double, or float for the fp32 factor of
// the mixed-precision path): L is converted on load, vectors and arithmetic are fp64 either way.
template <class TL>
__global__ __launch_bounds__(64) void k_solve_dinv(const TL *__restrict__ base, const chol_trsv_desc *__restrict__ descs, double *__restrict__ W)
{ // grid (separators of the level, 16-column blocks of the widest one)
  __shared__ double sYd[4][TS];
  const chol_trsv_desc d = descs[blockIdx.x];
  const int j0 = blockIdx.y * TS;
  if (j0 >= d.n) return;
  const TL *Lp = base + d.a_off;
  const int n = d.n, ldl = d.lda;
  const int lane = threadIdx.x, r15 = lane & 15, g = lane >> 4;
  const int row = j0 + r15, b4 = r15 & ~3, qi = r15 & 3;
  double blk[4], x[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int col = j0 + b4 + k;
    double v = (k == qi) ? 1.0 : 0.0; // identity padding past n
    if (row < n && col < n) v = (k <= qi) ? (double)Lp[row + (int64_t)col * ldl] : 0.0;
    blk[k] = v;
  }
  double diag = blk[0];
  diag = (qi == 1) ? blk[1] : diag;
  diag = (qi == 2) ? blk[2] : diag;
  diag = (qi == 3) ? blk[3] : diag;
  linv4_quad(blk, 1.0 / diag, x, qi);
  if (lane < TS) {
#pragma unroll
    for (int m = 0; m < 4; ++m) sYd[qi][b4 + m] = x[m];
  }
  __syncthreads();
  double Lr[3];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const int c = g + 4 * b;
    double v = (r15 == c) ? 1.0 : 0.0;
    if (row < n && j0 + c < n) v = (c <= r15) ? (double)Lp[row + (int64_t)(j0 + c) * ldl] : 0.0;
    Lr[b] = v;
  }
  store_linv16(W + d.dinv_off + (int64_t)blockIdx.y * TS * TS, Lr, sYd[g][r15], r15, g);
}

// y_s <- L_ss^-1 y_s (forward) or L_ss^-T y_s (backward), one workgroup per separator, 64-column block steps:
// the block's triangle and its four 16x16 inverses go to LDS, wave 0 solves the block there, then every thread
// folds the solved block into the rows below (forward) / the block gathers the solved rows below first (backward)
// Only the columns [col0, col0 + SSPAN) of every separator are handled per launch: the rows below that span are folded
// in (forward) / gathered (backward) by k_solve_panel over all CUs, so a wide separator's triangle is not streamed by
// one workgroup.
#define SSPAN 256
// sL: [r][c] of the current diagonal block; sxs: the span's part of the vector, in LDS from the first block to the last.  PUB: the solution is written with
// agent-scope stores (workgroups of the same launch read it: k_solve_step)
template <bool BWD, class TL, bool PUB, bool XAG = false>
__device__ __forceinline__ void trsv_body(const TL *__restrict__ base, const chol_trsv_desc &d, const double *__restrict__ Wall, double *__restrict__ y, int col0,
                                          double (*sL)[SNB + 1], double (*sW)[TS * TS], double *sxs)
{
  const TL *Lm = base + d.a_off;
  const double *W = Wall + d.dinv_off;
  double *x = y + d.x_off;
  const int lda = d.lda, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (d.n <= col0) return;
  const int n = min(d.n, col0 + SSPAN); // rows and columns of this launch's span
  const int nblk = (n - col0 + SNB - 1) / SNB;
  // The span is a chain of (at most) four 64-column blocks: in-block solve on wave 0, then the fold of the block into the span's other rows (forward:
  // the rows below, x[r] -= L(r, J) x_J; backward: the columns in front, x[c] -= L(J, c)^T x_J).  Nothing the chain reads from memory depends on x,
  // and a 256-thread workgroup alone on its CU owns 512 registers per lane: EVERY load of the span -- the four triangles, their 16x16 inverses and
  // the six fold passes -- is requested before the first block is solved, so the span costs one memory round trip instead of three per block
  // (100 spans per direction at 100^3 are the critical path of a solve: 62 / 71 us per span in profiles/r3, forward / backward, before this).
  constexpr int NB4 = SSPAN / SNB, NL = SNB * SNB / 256, NW = (SNB / TS) * TS * TS / 256, NF = NB4 * (NB4 - 1) / 2;
  static_assert(SSPAN == 256 && NB4 == 4, "one thread per span row, four blocks");
  TL lv[NB4][NL], fa[NF][16];
  double wv[NB4][NW];
  const int fi = tid >> 2, part = tid & 3; // fold: four threads per row (forward) / column (backward), sixteen elements each
#pragma unroll
  for (int bi = 0; bi < NB4; ++bi) {
    if (bi >= nblk) break;
    const int J0 = col0 + (BWD ? nblk - 1 - bi : bi) * SNB, jb = min(SNB, n - J0);
#pragma unroll
    for (int u = 0; u < NL; ++u) { // (clamped addresses: a partial block reads its last row / column again)
      const int e = tid + 256 * u, r = e & (SNB - 1), c = e >> 6;
      lv[bi][u] = Lm[(J0 + min(r, jb - 1)) + (int64_t)(J0 + min(c, jb - 1)) * lda];
    }
#pragma unroll
    for (int u = 0; u < NW; ++u) {
      const int e = tid + 256 * u, t = min(e >> 8, (jb - 1) / TS);
      wv[bi][u] = W[(int64_t)(J0 / TS + t) * TS * TS + (e & 255)];
    }
#pragma unroll
    for (int p = 0; p < NB4 - 1 - bi; ++p) { // the bi-th block of the chain has at most 3 - bi blocks of 64 rows / columns to fold into
      const int f = bi * (NB4 - 1) - bi * (bi - 1) / 2 + p;
      if (BWD) {
        const int c = col0 + 64 * p + fi; // a column in front of the block (every block in front of another one is full)
        if (col0 + 64 * p < J0) {
#pragma unroll
          for (int u = 0; u < 16; ++u) fa[f][u] = Lm[J0 + min(16 * part + u, jb - 1) + (int64_t)c * lda];
        }
      } else {
        const int r0 = J0 + jb + 64 * p;
        if (r0 < n) {
#pragma unroll
          for (int u = 0; u < 16; ++u) fa[f][u] = Lm[min(r0 + fi, n - 1) + (int64_t)(J0 + min(16 * part + u, jb - 1)) * lda];
        }
      }
    }
  }
  sxs[tid] = col0 + tid < n ? gload<XAG>(&x[col0 + tid]) : 0.0;
#pragma unroll
  for (int bi = 0; bi < NB4; ++bi) {
    if (bi >= nblk) break;
    const int J0 = col0 + (BWD ? nblk - 1 - bi : bi) * SNB, jb = min(SNB, n - J0);
    double *const sx = sxs + (J0 - col0); // the block's right-hand side, then its solution (the blocks solved before it have folded themselves in)
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int e = tid + 256 * u, r = e & (SNB - 1), c = e >> 6;
      sL[r][c] = (r < jb && c <= r) ? (double)lv[bi][u] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < NW; ++u) { const int e = tid + 256 * u; sW[e >> 8][e & 255] = wv[bi][u]; }
    __syncthreads();
    if (wave == 0) { // in-block solve with the 16x16 inverses, lane = row of the block.  The sub-block's right-hand side and solution go
                     // through sx (LDS executes a wave's accesses in order; every lane reads them back as broadcasts): sixteen shuffles of a value
                     // that the same loop updates were sixteen dependent LDS-crossbar round trips per sub-block and loop -- most of the span's time
      double v = sx[lane];
      const int nsub = (jb + TS - 1) / TS, g4 = lane >> 4, r16 = lane & 15;
      for (int su = 0; su < nsub; ++su) {
        const int j = BWD ? nsub - 1 - su : su;
        if (g4 == j) sx[lane] = v; // the sub-block's right-hand side, the earlier sub-blocks folded in
        // x_j = Linv_j v_j (forward) / Linv_j^T v_j (backward); sW[j][k * 16 + c] = Linv(c, k)
        double xj = 0.0;
#pragma unroll
        for (int k = 0; k < TS; ++k) xj += (BWD ? sW[j][r16 * TS + k] : sW[j][k * TS + r16]) * sx[j * TS + k];
        if (g4 == j) sx[lane] = xj;
        // fold x_j into the rest of the block: every lane forms its dot product (unconditional LDS reads: they batch behind one wait; inside a
        // per-lane-group branch each of the sixteen was a branch, two reads and a wait of its own), the lanes it concerns subtract it
        double fd = 0.0;
#pragma unroll
        for (int k = 0; k < TS; ++k) fd += (BWD ? sL[j * TS + k][lane] : sL[lane][j * TS + k]) * sx[j * TS + k];
        if (BWD ? g4 < j : g4 > j) v -= fd;
      }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < NB4 - 1 - bi; ++p) {
      const int f = bi * (NB4 - 1) - bi * (bi - 1) / 2 + p;
      const int tgt = BWD ? 64 * p + fi : (J0 - col0) + jb + 64 * p + fi; // the target row / column inside the span
      const bool live = BWD ? col0 + 64 * p < J0 : J0 + jb + 64 * p < n;
      if (live) {
        double acc = 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += (16 * part + u < jb) ? (double)fa[f][u] * sx[16 * part + u] : 0.0;
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        if (part == 0 && col0 + tgt < n) sxs[tgt] -= acc;
      }
    }
    __syncthreads(); // the block's folds are in LDS (the next block's right-hand side), sL / sW may be rewritten
  }
  if (col0 + tid < n) gstore<PUB>(&x[col0 + tid], sxs[tid]);
}
template <bool BWD, class TL>
__global__ __launch_bounds__(256) void k_solve_trsv(const TL *__restrict__ base, const chol_trsv_desc *__restrict__ descs, const double *__restrict__ Wall,
                                                    double *__restrict__ y, int col0)
{
  __shared__ double sL[SNB][SNB + 1];
  __shared__ double sW[SNB / TS][TS * TS];
  __shared__ double sxs[SSPAN];
  trsv_body<BWD, TL, false>(base, descs[blockIdx.x], Wall, y, col0, sL, sW, sxs);
}
// The diagonal solve of one 256-column span out of an fp32 factor (round 4; the spans of the wide top separators are two thirds of a solve at 100^3: 101 per
// direction, 23 / 26 us each in k_solve_trsv).  One thread per row (forward) / column (backward) of the span; EVERY entry of the span's triangle the thread
// will need -- its row left of its own 16-block, or its column below it: up to 240 floats -- is requested before the first block is solved (a 256-thread
// workgroup alone on its CU owns 512 registers per lane), and so is its block's 16x16 inverse.  Then sixteen block steps with ONE barrier each: the sixteen
// lanes that hold block j's right-hand side form x_j = Linv_j r_j in registers (sixteen DPP multiply-adds: lane k of the row supplies r_k), publish it in
// LDS, and every thread on the far side of the block subtracts its sixteen products.  No triangle in LDS, no shuffles, no second barrier: the next block's
// lanes go on from their own registers.
// PUB: the solution is written with agent-scope stores -- workgroups of the same launch read it (k_solve_step); XAG: the right-hand side is read with
// agent-scope loads -- atomics of this launch have touched it (k_solve_leaf32)
template <bool BWD, bool PUB, bool XAG = false>
__device__ __forceinline__ void span32_body(const float *__restrict__ base, const chol_trsv_desc &d, const double *__restrict__ Wall, double *__restrict__ y, int col0, double *sx)
{
  const int lda = d.lda, tid = threadIdx.x, myb = tid >> 4, l16 = tid & 15;
  const int ns = min(d.n - col0, SSPAN), nb = (ns + TS - 1) / TS;
  const float *Lm = base + d.a_off + col0 + (int64_t)col0 * lda; // element (0, 0) of the span's diagonal block
  const double *Wb = Wall + d.dinv_off + (int64_t)(col0 / TS + min(myb, nb - 1)) * TS * TS; // Wb[k * 16 + c] = Linv(c, k) of the thread's own block
  double *x = y + d.x_off + col0;
  float lrow[(SSPAN / TS - 1) * TS], ltail[TS];
  double wl[TS];
  const bool live = tid < ns;
  const int nfull = ns / TS; // blocks of sixteen whole rows; block nfull (if nfull < nb) is the ragged one
#pragma unroll
  for (int k = 0; k < TS; ++k) wl[k] = BWD ? Wb[l16 * TS + k] : Wb[k * TS + l16]; // forward: Linv(l, k); backward: Linv(k, l)
  double r = live ? gload<XAG>(&x[tid]) : 0.0;
  if (!BWD) { // row tid: the columns of the blocks in front of its own
    const float *Lr = Lm + tid;
#pragma unroll
    for (int j = 0; j < SSPAN / TS - 1; ++j) {
      if (live && j < myb) {
#pragma unroll
        for (int k = 0; k < TS; ++k) lrow[j * TS + k] = Lr[(int64_t)(j * TS + k) * lda];
      } else {
#pragma unroll
        for (int k = 0; k < TS; ++k) lrow[j * TS + k] = 0.0f;
      }
    }
  } else { // column tid: the rows of the blocks below its own (slot j - 1 = block j); sixteen consecutive floats per block: 16-byte loads
    const float *Lc = Lm + (int64_t)min(tid, ns - 1) * lda;
#pragma unroll
    for (int j = 1; j < SSPAN / TS; ++j) {
      if (live && j > myb && j < nfull) {
#pragma unroll
        for (int k4 = 0; k4 < TS; k4 += 4) {
          const float4 v = *(const float4 *)&Lc[j * TS + k4];
          lrow[(j - 1) * TS + k4] = v.x; lrow[(j - 1) * TS + k4 + 1] = v.y; lrow[(j - 1) * TS + k4 + 2] = v.z; lrow[(j - 1) * TS + k4 + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int k = 0; k < TS; ++k) lrow[(j - 1) * TS + k] = 0.0f;
      }
    }
#pragma unroll
    for (int k = 0; k < TS; ++k) { // the ragged last block: its rows past the span's end do not exist (clamped address, zero value)
      const int row = nfull * TS + k;
      const float v = Lc[min(row, ns - 1)];
      ltail[k] = (live && nfull > myb && row < ns) ? v : 0.0f;
    }
  }
#pragma unroll
  for (int jb = 0; jb < SSPAN / TS; ++jb) {
    const int j = BWD ? SSPAN / TS - 1 - jb : jb; // compile time: the register indices below are constants
    if (j < nb) {
      if (myb == j) { // the block's own sixteen lanes: x_j = Linv_j r_j (backward: its transpose), lane k of the row supplies r_k
        double xj = 0.0;
#define SPAN_FM(K_) fmac_bcast<K_, K_ == 0>(xj, r, wl[K_]);
        SPAN_FM(0) SPAN_FM(1) SPAN_FM(2) SPAN_FM(3) SPAN_FM(4) SPAN_FM(5) SPAN_FM(6) SPAN_FM(7)
        SPAN_FM(8) SPAN_FM(9) SPAN_FM(10) SPAN_FM(11) SPAN_FM(12) SPAN_FM(13) SPAN_FM(14) SPAN_FM(15)
#undef SPAN_FM
        r = xj;
        sx[tid] = xj;
      }
      __syncthreads();
      if (BWD ? myb < j : myb > j) {
        double xv[TS], acc0 = 0.0, acc1 = 0.0; // the block's solution in eight 16-byte LDS reads, all in flight at once; two chains of eight multiply-adds
#pragma unroll
        for (int k = 0; k < TS; k += 2) {
          const double2 t = *(const double2 *)&sx[j * TS + k];
          xv[k] = t.x; xv[k + 1] = t.y;
        }
#pragma unroll
        for (int k = 0; k < TS; ++k) { // the value stays a float in its register until here: a conversion hoisted to the load would wait for it there
          float v = (BWD && j == nfull) ? ltail[k] : lrow[(BWD ? j - 1 : j) * TS + k];
          asm("" : "+v"(v));
          if (k & 1) acc1 += (double)v * xv[k]; else acc0 += (double)v * xv[k];
        }
        r -= acc0 + acc1;
      }
    }
  }
  if (live) gstore<PUB>(&x[tid], r);
}
template <bool BWD>
__global__ __launch_bounds__(256) void k_solve_span32(const float *__restrict__ base, const chol_trsv_desc *__restrict__ descs, const double *__restrict__ Wall,
                                                      double *__restrict__ y, int col0)
{
  __shared__ __attribute__((aligned(16))) double sx[SSPAN];
  const chol_trsv_desc d = descs[blockIdx.x];
  if (d.n <= col0) return;
  span32_body<BWD, false>(base, d, Wall, y, col0, sx);
}

// ---- column sums over a wave without the LDS crossbar (round 4) ----
// The backward sweep needs sum_i L(i, c) x(i) with the rows i along the lanes (the coalesced direction of a column-major panel): a reduction over the 64
// lanes per column.  Six __shfl_down stages per column are twelve ds_bpermute_b32 each, and the one LDS pipe of a CU bounded the whole backward sweep
// (2.4 TB/s on the leaf level of 100^3, 1.47 ms of an 11 ms solve).  gfx950 swaps half-waves and 16-lane rows BETWEEN two registers in one VALU
// instruction (v_permlane32_swap, v_permlane16_swap): two columns' partial sums fold into one register per stage, so sixteen columns cost 8 + 4 swaps-and-adds
// and four registers of four 16-lane rows, each finished by four DPP rotations -- 84 VALU instructions on four SIMDs in place of 192 bpermutes on one pipe.
typedef unsigned chol_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double fold32(double a, double b)
{ // lanes 0-31: a(l) + a(l + 32); lanes 32-63: b(l - 32) + b(l)
  const chol_u2 lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  const chol_u2 hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  return __hiloint2double((int)hi.x, (int)lo.x) + __hiloint2double((int)hi.y, (int)lo.y);
}
__device__ __forceinline__ double fold16(double a, double b)
{ // 16-lane rows: (a.row0 + a.row1, b.row0 + b.row1, a.row2 + a.row3, b.row2 + b.row3)
  const chol_u2 lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  const chol_u2 hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  return __hiloint2double((int)hi.x, (int)lo.x) + __hiloint2double((int)hi.y, (int)lo.y);
}
template <int CTRL> __device__ __forceinline__ double dpp_mov64(double v)
{
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double row_sum16(double v)
{ // every lane: the sum over its 16-lane row
  v += dpp_mov64<0x128>(v); // row_ror:8
  v += dpp_mov64<0x124>(v); // row_ror:4
  v += dpp_mov64<0x4e>(v);  // quad_perm [2,3,0,1]
  v += dpp_mov64<0xb1>(v);  // quad_perm [1,0,3,2]
  return v;
}
// the sums over all 64 lanes of acc[0..15]: lane l with (l & 15) < 4 returns the sum of column wave_sum16_col(l); the other lanes return junk
__device__ __forceinline__ int wave_sum16_col(int lane) { return 4 * (lane & 3) + ((lane >> 5) & 1) + 2 * ((lane >> 4) & 1); }
__device__ __forceinline__ double wave_sum16(const double (&acc)[16], int lane)
{
  double t[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { // rows of t[i]: columns 4 i + (0, 2, 1, 3)
    const double s0 = fold32(acc[4 * i], acc[4 * i + 1]), s1 = fold32(acc[4 * i + 2], acc[4 * i + 3]);
    t[i] = row_sum16(fold16(s0, s1));
  }
  const int i = lane & 3;
  return i == 0 ? t[0] : i == 1 ? t[1] : i == 2 ? t[2] : t[3];
}
// y(c) -= sum over the chunk's rows of A(i, c) x(i) for the columns [0, ncols) of a column-major block: `A` points at (first row of the chunk, column 0),
// `mrows` rows of the chunk exist (<= 64 PER), xa[u] = x(row lane + 64 u) (0 past the end).  Wave `wave` of four takes the columns 16 (wave + 4 k) ..+15:
// 16 PER loads in flight per lane, one wave_sum16 and ONE atomic instruction (16 lanes) per sixteen columns.
template <int PER, class TL>
__device__ __forceinline__ void gather_columns(const TL *__restrict__ A, int lda, int mrows, int ncols, const double (&xa)[PER], double *__restrict__ yc, int lane, int wave)
{
  int ro[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) ro[u] = min(lane + 64 * u, mrows - 1);
  for (int c0 = 16 * wave; c0 < ncols; c0 += 64) {
    TL a[16][PER];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const TL *Ac = A + (int64_t)min(c0 + q, ncols - 1) * lda;
#pragma unroll
      for (int u = 0; u < PER; ++u) a[q][u] = Ac[ro[u]]; // unconditional (clamped rows repeat the last one, x = 0 there): a predicate here serialises the loads
    }
    double acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      acc[q] = (double)a[q][0] * xa[0];
#pragma unroll
      for (int u = 1; u < PER; ++u) acc[q] += (double)a[q][u] * xa[u];
    }
    const double sum = wave_sum16(acc, lane);
    const int c = c0 + wave_sum16_col(lane);
    if ((lane & 15) < 4 && c < ncols) unsafeAtomicAdd(&yc[c], -sum);
  }
}

// rows of a wide separator under a span that one workgroup of k_solve_panel folds / gathers.  The spans of the top separators are the solve's chain and
// at the root there is ONE separator: with 512-row chunks a span step of the 10^4-column root kept 10 CUs busy on average
#ifndef SPANEL_BW_ROWS
#define SPANEL_BW_ROWS 128
#endif
#define SPANEL_FW_ROWS 256
template <bool BWD, class TL>
__global__ __launch_bounds__(256) void k_solve_panel(const TL *__restrict__ base, const chol_trsv_desc *__restrict__ descs, double *__restrict__ y, int col0)
{
  __shared__ double sx[SSPAN];
  const chol_trsv_desc d = descs[blockIdx.x];
  const int r0 = col0 + SSPAN;
  const int rows = BWD ? SPANEL_BW_ROWS : SPANEL_FW_ROWS;
  const int n = d.band > 0 ? min(d.n, r0 + d.band) : d.n; // a banded (leaf) block: the rows from r0 + band on are zero under these columns
  if (n <= r0 + (int)blockIdx.y * rows) return;
  const TL *Lm = base + d.a_off;
  double *x = y + d.x_off;
  const int lda = d.lda, tid = threadIdx.x;
  if (!BWD) {
    sx[tid] = x[col0 + tid];
    __syncthreads();
    const int r = r0 + blockIdx.y * 256 + tid;
    const TL *A = Lm + min(r, n - 1) + (int64_t)col0 * lda;
    double acc = 0.0;
    for (int k = 0; k < SSPAN; k += 32) { // thirty-two loads in flight per thread
      TL a[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) a[u] = A[(int64_t)(k + u) * lda];
#pragma unroll
      for (int u = 0; u < 32; ++u) acc += (double)a[u] * sx[k + u];
    }
    if (r < n) x[r] -= acc;
  } else {
    const int lane = tid & 63, wave = tid >> 6;
    constexpr int PER = SPANEL_BW_ROWS / 64;
    const int row0 = r0 + blockIdx.y * SPANEL_BW_ROWS;
    double xa[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int i = row0 + lane + 64 * u;
      xa[u] = i < n ? x[i] : 0.0;
    }
    gather_columns<PER>(Lm + row0 + (int64_t)col0 * lda, lda, min(n - row0, SPANEL_BW_ROWS), SSPAN, xa, x + col0, lane, wave);
  }
}

// One step of the span chain of the few wide separators at the top of the tree (fp32 factor) in ONE launch.  Launch by launch a step was: solve span k (one
// workgroup, ~10 us), then its whole panel (all CUs, ~12 us) -- but the next span needs only SSPAN rows of that panel.  Roles by blockIdx.y:
//   0                 the solve of span k (span32_body; publishes x_k with agent-scope stores, then the separator's flag = gen)
//   1 .. STEP_NB      the SSPAN rows / columns the NEXT span needs of span k's panel: their L entries are requested first, then the workgroup waits for the
//                     flag (the producer has the lowest block index of the launch and waits for nobody; the spin is bounded all the same: it poisons its
//                     part of the vector with NaN if it gives up), reads x_k with agent-scope loads and adds its part atomically
//   STEP_NB + 1 ..    the rest of the PREVIOUS span's panel (forward: rows behind span k under span k - 1; backward: the rows behind span k into the columns of
//                     span k - 1): everything it reads was final before the launch, it runs beside the solve
// so the chain per step is solve + flag + 1/16 of a SSPAN x SSPAN block instead of solve + launch + panel.
#define STEP_NB 16
#define STEP_MAX_SEPS 8    /* k_solve_step: a 512-register workgroup per role */
#define STEP_MAX_SEPS_W 128 /* k_solve_stepw (explicit span inverses): ordinary workgroups; = CHOL_STEPW_MAX_SEPS of chol_kernels.h (flags, scratch, inverses) */
static_assert(STEP_MAX_SEPS_W == CHOL_STEPW_MAX_SEPS, "flags and scratch of the step launches are sized by chol_kernels.h");
// A level of banded LEAVES (fp32 factor): the whole triangle of a leaf by ONE workgroup in ONE launch.  A leaf's factor stays inside the envelope of A, and
// with a band of at most SSPAN rows the panel under a span is a corner of the NEXT span's rows only: span by span the workgroup solves the span out of
// registers (span32_body) and folds it into / gathers from those <= 256 rows itself.  Launch by launch the 512 leaves of 100^3 took 6 span launches (512
// workgroups of one per CU: two rounds each) and 5 panel launches per sweep: 1.1 of the 7.1 ms of a solve.  Inside the launch the vector is written with
// agent-scope stores and read with agent-scope loads (the gather's atomics are performed in L2: a plain load could hit a line the CU cached before them).
template <bool BWD, class TL> struct leaf_span;
template <bool BWD> struct leaf_span<BWD, float> {
  static __device__ __forceinline__ void run(const float *base, const chol_trsv_desc &d, const double *Wall, double *y, int col0, double *sx) { span32_body<BWD, true, true>(base, d, Wall, y, col0, sx); }
};
template <bool BWD> struct leaf_span<BWD, double> { // (the fp64 factor: the 64-column block chain of k_solve_trsv)
  static __device__ __forceinline__ void run(const double *base, const chol_trsv_desc &d, const double *Wall, double *y, int col0, double *sx)
  {
    __shared__ double sL[SNB][SNB + 1];
    __shared__ double sW[SNB / TS][TS * TS];
    trsv_body<BWD, double, true, true>(base, d, Wall, y, col0, sL, sW, sx);
  }
};
template <bool BWD, class TL>
__global__ __launch_bounds__(256) void k_solve_leaf32(const TL *__restrict__ base, const chol_trsv_desc *__restrict__ descs, const double *__restrict__ Wall,
                                                      double *__restrict__ y)
{
  __shared__ __attribute__((aligned(16))) double sx[SSPAN];
  const chol_trsv_desc d = descs[blockIdx.x];
  const int n = d.n, lda = d.lda, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nspan = (n + SSPAN - 1) / SSPAN, band = d.band > 0 ? d.band : n;
  const TL *Lm = base + d.a_off;
  double *x = y + d.x_off;
  for (int i = 0; i < nspan; ++i) {
    const int sp = BWD ? nspan - 1 - i : i, col0 = sp * SSPAN, r0 = col0 + SSPAN;
    const int nr = min(n, r0 + band) - r0; // rows under the span inside the band (<= SSPAN; <= 0: none)
    if (BWD && nr > 0) { // x(span) -= L(rows under it, span)^T x(rows): the rows are the head of the span solved before this one
      double xa[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) xa[u] = lane + 64 * u < nr ? gload<true>(&x[r0 + lane + 64 * u]) : 0.0;
      gather_columns<4>(Lm + r0 + (int64_t)col0 * lda, lda, nr, SSPAN, xa, x + col0, lane, wave);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    leaf_span<BWD, TL>::run(base, d, Wall, y, col0, sx);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!BWD && nr > 0) { // x(rows under the span) -= L(rows, span) x(span)
      sx[tid] = gload<true>(&x[col0 + tid]);
      __syncthreads();
      const TL *A = Lm + r0 + min(tid, nr - 1) + (int64_t)col0 * lda;
      double acc = 0.0;
      for (int k = 0; k < SSPAN; k += 64) { // (the span's registers are free again: sixty-four loads in flight, four rounds)
        TL a[64];
#pragma unroll
        for (int u = 0; u < 64; ++u) a[u] = A[(int64_t)(k + u) * lda];
#pragma unroll
        for (int u = 0; u < 64; ++u) acc += (double)a[u] * sx[k + u];
      }
      if (tid < nr) gstore<true>(&x[r0 + tid], gload<true>(&x[r0 + tid]) - acc);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  }
}

template <bool BWD, class TL> struct step_span;
template <bool BWD> struct step_span<BWD, float> {
  static __device__ __forceinline__ void run(const float *base, const chol_trsv_desc &d, const double *Wall, double *y, int col0, double *sx) { span32_body<BWD, true>(base, d, Wall, y, col0, sx); }
};
template <bool BWD> struct step_span<BWD, double> { // the fp64 factor's span: the 64-column block chain of k_solve_trsv
  static __device__ __forceinline__ void run(const double *base, const chol_trsv_desc &d, const double *Wall, double *y, int col0, double *sx)
  {
    __shared__ double sL[SNB][SNB + 1];
    __shared__ double sW[SNB / TS][TS * TS];
    trsv_body<BWD, double, true>(base, d, Wall, y, col0, sL, sW, sx);
  }
};
template <bool BWD, class TL>
__global__ __launch_bounds__(256) void k_solve_step(const TL *__restrict__ base, const chol_trsv_desc *__restrict__ descs, const double *__restrict__ Wall,
                                                    double *__restrict__ y, int col0, int *__restrict__ flags, int gen)
{
  __shared__ __attribute__((aligned(16))) double sx[SSPAN];
  const chol_trsv_desc d = descs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lda = d.lda, n = d.n;
  const int role = blockIdx.y;
  if (n <= col0) return; // (every role of a separator without this span)
  const TL *Lm = base + d.a_off;
  double *x = y + d.x_off;
  if (role == 0) {
    step_span<BWD, TL>::run(base, d, Wall, y, col0, sx);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_store(&flags[blockIdx.x], gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if (role <= STEP_NB) {
    const int part = role - 1;
    bool ok = true;
    if (!BWD) { // rows col0 + SSPAN + 16 part .. + 15 under the columns of span k: thread (row, sixteenth of the columns)
      const int r = tid & 15, kp = tid >> 4, row = col0 + SSPAN + TS * part + r;
      if (col0 + SSPAN + TS * part >= n) return;
      const TL *A = Lm + min(row, n - 1) + (int64_t)(col0 + TS * kp) * lda;
      TL a[TS];
#pragma unroll
      for (int u = 0; u < TS; ++u) a[u] = A[(int64_t)u * lda];
      if (tid < 64) {
        int v = 0, it = 0;
        for (; it < (1 << 22); ++it) {
          v = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&flags[blockIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
          if (v == gen) break;
          __builtin_amdgcn_s_sleep(4);
        }
        if (tid == 0) ((int *)sx)[0] = v == gen;
      }
      __syncthreads();
      ok = ((volatile int *)sx)[0] != 0;
      __syncthreads();
      double acc = 0.0;
#pragma unroll
      for (int u = 0; u < TS; ++u) acc += (double)a[u] * gload<true>(&x[col0 + TS * kp + u]);
      sx[kp * TS + r] = acc;
      __syncthreads();
      if (tid < TS) {
        double sum = 0.0;
#pragma unroll
        for (int q = 0; q < TS; ++q) sum += sx[q * TS + tid];
        if (!ok) sum = __builtin_nan("");
        if (row < n) unsafeAtomicAdd(&x[row], -sum);
      }
    } else { // the rows of span k into the columns col0 - SSPAN + 16 part .. + 15 of span k - 1: wave w the rows 64 w .. 64 w + 63
      if (col0 == 0) return;
      const int c0 = col0 - SSPAN + TS * part, ns = min(n - col0, SSPAN), row = 64 * wave + lane;
      const TL *A = Lm + col0 + min(row, ns - 1) + (int64_t)c0 * lda;
      TL a[TS];
#pragma unroll
      for (int q = 0; q < TS; ++q) a[q] = A[(int64_t)q * lda];
      if (tid < 64) {
        int v = 0, it = 0;
        for (; it < (1 << 22); ++it) {
          v = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&flags[blockIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
          if (v == gen) break;
          __builtin_amdgcn_s_sleep(4);
        }
        if (tid == 0) ((int *)sx)[0] = v == gen;
      }
      __syncthreads();
      ok = ((volatile int *)sx)[0] != 0;
      const double xr = row < ns ? gload<true>(&x[col0 + row]) : 0.0;
      double acc[TS];
#pragma unroll
      for (int q = 0; q < TS; ++q) acc[q] = (double)a[q] * xr;
      double sum = wave_sum16(acc, lane);
      if (!ok) sum = __builtin_nan("");
      if ((lane & 15) < 4) unsafeAtomicAdd(&x[c0 + wave_sum16_col(lane)], -sum);
    }
    return;
  }
  // the rest of the previous span's panel
  if (col0 == 0) return;
  const int chunk = role - STEP_NB - 1, pc0 = col0 - SSPAN, r0 = col0 + SSPAN;
  if (!BWD) {
    if (n <= r0 + chunk * SPANEL_FW_ROWS) return;
    sx[tid] = x[pc0 + tid];
    __syncthreads();
    const int r = r0 + chunk * SPANEL_FW_ROWS + tid;
    const TL *A = Lm + min(r, n - 1) + (int64_t)pc0 * lda;
    double acc = 0.0;
    for (int k = 0; k < SSPAN; k += 32) {
      TL a[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) a[u] = A[(int64_t)(k + u) * lda];
#pragma unroll
      for (int u = 0; u < 32; ++u) acc += (double)a[u] * sx[k + u];
    }
    if (r < n) unsafeAtomicAdd(&x[r], -acc); // (the rows of the next span also receive the middle role's sums)
  } else {
    constexpr int PER = SPANEL_BW_ROWS / 64;
    const int row0 = r0 + chunk * SPANEL_BW_ROWS;
    if (n <= row0) return;
    double xa[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int i = row0 + lane + 64 * u;
      xa[u] = i < n ? x[i] : 0.0;
    }
    gather_columns<PER>(Lm + row0 + (int64_t)pc0 * lda, lda, min(n - row0, SPANEL_BW_ROWS), SSPAN, xa, x + pc0, lane, wave);
  }
}

// ---- the span chain of the wide top separators with EXPLICIT inverses of the 256 x 256 diagonal spans (round 4) ----
// k_solve_step's chain per span is the span solve itself: 10-15 us of sixteen dependent 16-column block steps in one workgroup.  With inv(L_kk) at hand
// (k_solve_inv256, once per solve: the factor's 16x16 inverses doubled up block column by block column on the matrix cores) x_k = inv(L_kk) r_k is a
// 256 x 256 triangular matrix-vector product with NO chain: sixteen workgroups take sixteen rows (forward) / columns (backward) each, reading a right-hand
// side that was final before the launch.  Roles by blockIdx.y:
//   0 .. 15    part p of x_k into the separator's scratch vector xt (the right-hand side must stay until every part has read it), then flag p = gen
//   16 .. 31   wait for all sixteen flags; copy part p of xt into the vector; the SSPAN rows / columns the next span needs of span k's panel (as k_solve_step's
//              middle role, with x_k from xt)
//   32 ..      the rest of the previous span's panel (as k_solve_step)
// W256: [column][row] (column-major, 256 x 256 doubles per span), lower triangle in 16 x 16 blocks; blocks above the diagonal are never written or read.
template <class TL>
__global__ __launch_bounds__(64) void k_solve_inv256(const TL *__restrict__ base, const chol_trsv_desc *__restrict__ descs, const double *__restrict__ W16all,
                                                     double *__restrict__ W256, int nspan_max)
{ // one wave per (separator, span, block column j): X(i, j) = -inv(L_ii) sum_{k = j .. i-1} L(i, k) X(k, j), X(j, j) = inv(L_jj); the column's blocks stay in the
  // wave's registers in the fp64 MFMA result layout (register q of lane (n, g): row g + 4 q, column n), which is also the layout of the next product's second
  // operand with k = g + 4 s in instruction s
  const chol_trsv_desc d = descs[blockIdx.x];
  const int sp = blockIdx.y, j = blockIdx.z, col0 = sp * SSPAN;
  if (d.n <= col0) return;
  const int ns = min(d.n - col0, SSPAN), nb = (ns + TS - 1) / TS;
  if (j >= nb) return;
  const int lane = threadIdx.x, n16 = lane & 15, g = lane >> 4, lda = d.lda;
  const TL *Lm = base + d.a_off + col0 + (int64_t)col0 * lda;
  const double *W16 = W16all + d.dinv_off + (int64_t)(col0 / TS) * TS * TS; // W16[b * 256 + c * 16 + r] = inv(L_bb)(r, c)
  double *out = W256 + ((int64_t)blockIdx.x * nspan_max + sp) * (SSPAN * SSPAN) + (int64_t)(TS * j + n16) * SSPAN + g;
  d4 X[SSPAN / TS];
#pragma unroll
  for (int i = 0; i < SSPAN / TS; ++i) X[i] = (d4){ 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
  for (int i = 0; i < SSPAN / TS; ++i) {
    if (i == j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) X[i][q] = W16[i * TS * TS + n16 * TS + g + 4 * q];
    } else if (i > j && i < nb) {
      d4 S = { 0.0, 0.0, 0.0, 0.0 };
      const int row = min(TS * i + n16, ns - 1); // (first operand: lane = row of L(i, k))
#pragma unroll
      for (int k = 0; k < SSPAN / TS; ++k) {
        if (k >= j && k < i) {
#pragma unroll
          for (int s = 0; s < 4; ++s) S = __builtin_amdgcn_mfma_f64_16x16x4f64((double)Lm[row + (int64_t)(TS * k + g + 4 * s) * lda], X[k][s], S, 0, 0, 0);
        }
      }
      d4 D = { 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
      for (int s = 0; s < 4; ++s) D = __builtin_amdgcn_mfma_f64_16x16x4f64(W16[i * TS * TS + (g + 4 * s) * TS + n16], S[s], D, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) X[i][q] = -D[q];
    }
    if (i >= j && i < nb) {
#pragma unroll
      for (int q = 0; q < 4; ++q) out[TS * i + 4 * q] = X[i][q];
    }
  }
}
// every one of the sixteen flags equals gen (bounded; false: gave up)
__device__ __forceinline__ bool wait_parts16(const int *f, int gen, int tid, int *sflag)
{
  if (tid < 64) {
    bool ok = false;
    for (int it = 0; it < (1 << 22); ++it) {
      const int v = tid < STEP_NB ? __hip_atomic_load(&f[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : gen;
      if (__all(v == gen)) { ok = true; break; }
      __builtin_amdgcn_s_sleep(4);
    }
    if (tid == 0) *sflag = ok;
  }
  __syncthreads();
  const bool r = *(volatile int *)sflag != 0;
  __syncthreads();
  return r;
}
template <bool BWD, class TL>
__global__ __launch_bounds__(256) void k_solve_stepw(const TL *__restrict__ base, const chol_trsv_desc *__restrict__ descs, const double *__restrict__ W256,
                                                     int nspan_max, double *__restrict__ y, double *__restrict__ xtmp, int col0, int *__restrict__ flags, int gen)
{
  __shared__ __attribute__((aligned(16))) double sx[SSPAN];
  const chol_trsv_desc d = descs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lda = d.lda, n = d.n;
  const int role = blockIdx.y;
  if (n <= col0) return; // (every role of a separator without this span)
  const TL *Lm = base + d.a_off;
  double *x = y + d.x_off, *xt = xtmp + blockIdx.x * SSPAN;
  int *fl = flags + blockIdx.x * STEP_NB;
  const int ns = min(n - col0, SSPAN);
  if (role < STEP_NB) { // part `role` of x_k = inv(L_kk) r_k (forward: sixteen rows) / inv(L_kk)^T r_k (backward: sixteen columns)
    const int p = role, r = tid & 15, kp = tid >> 4;
    const double *W = W256 + ((int64_t)blockIdx.x * nspan_max + col0 / SSPAN) * (SSPAN * SSPAN);
    if (TS * p < ns) {
      double acc = 0.0;
      if (!BWD) { // thread (row 16 p + r, columns 16 kp .. + 15), the blocks left of the diagonal one and it
        if (kp <= p) {
          double w[TS], v[TS];
#pragma unroll
          for (int u = 0; u < TS; ++u) { w[u] = W[(int64_t)(TS * kp + u) * SSPAN + TS * p + r]; v[u] = x[col0 + min(TS * kp + u, ns - 1)]; }
#pragma unroll // (a ragged last block: the columns past the span are selected away, not multiplied by their zeros -- what lies behind the vector may be NaN)
          for (int u = 0; u < TS; ++u) acc += TS * kp + u < ns ? w[u] * v[u] : 0.0;
        }
        sx[kp * TS + r] = acc;
        __syncthreads();
        if (tid < TS) {
          double sum = 0.0;
#pragma unroll
          for (int q = 0; q < TS; ++q) sum += sx[q * TS + tid];
          if (TS * p + tid < ns) gstore<true>(&xt[TS * p + tid], sum);
        }
      } else { // thread (column 16 p + kp, rows 16 g + r of the blocks g >= p): sum over the sixteen lanes of a row
        const int c = TS * p + kp;
        if (c < ns) {
          const double *Wc = W + (int64_t)c * SSPAN;
          double w[SSPAN / TS], v[SSPAN / TS]; // unconditional loads (a predicate per load is a branch and a wait per load); what lies above the diagonal block
#pragma unroll                          // row or past the span is never written: selected away, not multiplied by zero
          for (int gq = 0; gq < SSPAN / TS; ++gq) { w[gq] = Wc[TS * gq + r]; v[gq] = x[col0 + min(TS * gq + r, ns - 1)]; }
#pragma unroll
          for (int gq = 0; gq < SSPAN / TS; ++gq) acc += (gq >= p && TS * gq + r < ns) ? w[gq] * v[gq] : 0.0;
        }
        acc = row_sum16(acc);
        if (r == 0 && c < ns) gstore<true>(&xt[c], acc);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_store(&fl[p], gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if (role < 2 * STEP_NB) {
    const int part = role - STEP_NB;
    if (!BWD) { // rows col0 + SSPAN + 16 part .. + 15 under the columns of span k: thread (row, sixteenth of the columns)
      const int r = tid & 15, kp = tid >> 4, row = col0 + SSPAN + TS * part + r;
      const bool rows = col0 + SSPAN + TS * part < n;
      TL a[TS];
      if (rows) {
        const TL *A = Lm + min(row, n - 1) + (int64_t)(col0 + TS * kp) * lda;
#pragma unroll
        for (int u = 0; u < TS; ++u) a[u] = A[(int64_t)u * lda];
      }
      const bool ok = wait_parts16(fl, gen, tid, (int *)sx);
      if (tid < TS && TS * part + tid < ns) gstore<true>(&x[col0 + TS * part + tid], ok ? gload<true>(&xt[TS * part + tid]) : __builtin_nan(""));
      if (!rows) return;
      double acc = 0.0;
#pragma unroll
      for (int u = 0; u < TS; ++u) acc += (double)a[u] * gload<true>(&xt[TS * kp + u]);
      sx[kp * TS + r] = acc;
      __syncthreads();
      if (tid < TS) {
        double sum = 0.0;
#pragma unroll
        for (int q = 0; q < TS; ++q) sum += sx[q * TS + tid];
        if (!ok) sum = __builtin_nan("");
        if (row < n) unsafeAtomicAdd(&x[row], -sum);
      }
    } else { // the rows of span k into the columns col0 - SSPAN + 16 part .. + 15 of span k - 1: wave w the rows 64 w .. 64 w + 63
      const int c0 = col0 - SSPAN + TS * part, row = 64 * wave + lane;
      TL a[TS];
      if (col0 > 0) {
        const TL *A = Lm + col0 + min(row, ns - 1) + (int64_t)c0 * lda;
#pragma unroll
        for (int q = 0; q < TS; ++q) a[q] = A[(int64_t)q * lda];
      }
      const bool ok = wait_parts16(fl, gen, tid, (int *)sx);
      if (tid < TS && TS * part + tid < ns) gstore<true>(&x[col0 + TS * part + tid], ok ? gload<true>(&xt[TS * part + tid]) : __builtin_nan(""));
      if (col0 == 0) return;
      const double xr = row < ns ? gload<true>(&xt[row]) : 0.0;
      double acc[TS];
#pragma unroll
      for (int q = 0; q < TS; ++q) acc[q] = (double)a[q] * xr;
      double sum = wave_sum16(acc, lane);
      if (!ok) sum = __builtin_nan("");
      if ((lane & 15) < 4) unsafeAtomicAdd(&x[c0 + wave_sum16_col(lane)], -sum);
    }
    return;
  }
  // the rest of the previous span's panel, in (row chunk) x (half of the span's columns) pieces: the launch is as long as its longest workgroup
  if (col0 == 0) return;
  const int chunk = (role - 2 * STEP_NB) >> 1, kh = (role - 2 * STEP_NB) & 1, pc0 = col0 - SSPAN + (SSPAN / 2) * kh, r0 = col0 + SSPAN;
  if (!BWD) {
    if (n <= r0 + chunk * SPANEL_FW_ROWS) return;
    if (tid < SSPAN / 2) sx[tid] = x[pc0 + tid];
    __syncthreads();
    const int r = r0 + chunk * SPANEL_FW_ROWS + tid;
    const TL *A = Lm + min(r, n - 1) + (int64_t)pc0 * lda;
    double acc = 0.0;
    for (int k = 0; k < SSPAN / 2; k += 32) {
      TL a[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) a[u] = A[(int64_t)(k + u) * lda];
#pragma unroll
      for (int u = 0; u < 32; ++u) acc += (double)a[u] * sx[k + u];
    }
    if (r < n) unsafeAtomicAdd(&x[r], -acc);
  } else {
    constexpr int PER = SPANEL_BW_ROWS / 64;
    const int row0 = r0 + chunk * SPANEL_BW_ROWS;
    if (n <= row0) return;
    double xa[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int i = row0 + lane + 64 * u;
      xa[u] = i < n ? x[i] : 0.0;
    }
    gather_columns<PER>(Lm + row0 + (int64_t)pc0 * lda, lda, min(n - row0, SPANEL_BW_ROWS), SSPAN / 2, xa, x + pc0, lane, wave);
  }
}

// forward: y_anc[rows] -= A(rows, cols) y_s for one (row chunk, column chunk) of the block A = (anc, s); y_s staged through LDS.  items = (block, first
// row, first column) triples: the column chunks (CHOL_SOLVE_COLS) give the few tall blocks of the top levels enough workgroups to fill the chip
template <class TL>
__global__ __launch_bounds__(256) void k_solve_gemv_fwd(const TL *__restrict__ base, const chol_gemv_desc *__restrict__ blocks, const int *__restrict__ items,
                                                        double *__restrict__ y)
{
  __shared__ double sx[256];
  const chol_gemv_desc d = blocks[items[4 * blockIdx.x]];
  const int r = items[4 * blockIdx.x + 1] + threadIdx.x, c0 = max(items[4 * blockIdx.x + 2], items[4 * blockIdx.x + 3]), c1 = min(d.n, items[4 * blockIdx.x + 2] + CHOL_SOLVE_COLS);
  if (c0 >= c1) return; // (the rows of a leaf's panel are zero in front of their first entry of A: items[.. + 3])
  const TL *A = base + d.a_off + min(r, d.m - 1);
  const double *xs = y + d.y_off; // the separator's (already solved) part
  double acc = 0.0;
  for (int k0 = c0; k0 < c1; k0 += 256) {
    const int kb = min(256, c1 - k0);
    __syncthreads();
    if ((int)threadIdx.x < kb) sx[threadIdx.x] = xs[k0 + threadIdx.x];
    __syncthreads();
    const TL *Ak = A + (int64_t)k0 * d.lda;
    int k = 0;
    for (; k + 32 <= kb; k += 32) { // thirty-two loads in flight per thread: with sixteen, 32 waves x 256 B x (the ~60 % of lanes a leaf's blocks fill) is
      TL a[32];                     // under the ~90 KB a CU must keep in flight for its share of HBM
#pragma unroll
      for (int u = 0; u < 32; ++u) a[u] = Ak[(int64_t)(k + u) * d.lda];
#pragma unroll
      for (int u = 0; u < 32; ++u) acc += (double)a[u] * sx[k + u];
    }
    for (; k + 16 <= kb; k += 16) {
      TL a[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) a[u] = Ak[(int64_t)(k + u) * d.lda];
#pragma unroll
      for (int u = 0; u < 16; ++u) acc += (double)a[u] * sx[k + u];
    }
    for (; k + 8 <= kb; k += 8) {
      double a[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] = (double)Ak[(int64_t)(k + u) * d.lda];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += a[u] * sx[k + u];
    }
    for (; k < kb; ++k) acc += (double)Ak[(int64_t)k * d.lda] * sx[k];
  }
  if (r < d.m) unsafeAtomicAdd(&y[d.x_off + r], -acc);
}

// backward: y_s[c] -= sum over the rows of the separator's panel below its diagonal block of A(i, c) y_anc(i).  One workgroup = 64 columns of ONE separator
// and a run of its row-run descriptors (q0 .. q1: all of them, unless the level has too few separators to fill the chip): the sums stay in registers
// over every block the separator has into its ancestors and reach y with ONE atomic per column per workgroup.  (Per (block, 512-row chunk) the leaf
// level of 100^3 issued 7 M fp64 atomics -- several row chunks and ~8 ancestor blocks per column, device-scope read-modify-writes that bounded the level at
// 1.47 ms whatever the reduction cost: swapping the shuffles for the swap-based sums above without merging changed nothing, more chunks made it worse.)
template <class TL>
__global__ __launch_bounds__(256) void k_solve_gather_bwd(const TL *__restrict__ base, const chol_gemv_desc *__restrict__ blocks, const int *__restrict__ items,
                                                          double *__restrict__ y)
{
  const int q0 = items[4 * blockIdx.x], q1 = items[4 * blockIdx.x + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cw = items[4 * blockIdx.x + 2] + 16 * wave, n = blocks[q0].n;
  if (cw >= n) return; // no barrier in this kernel
  const int ncol = min(16, n - cw);
  constexpr int PER = 4;
  double acc[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.0;
  for (int b = q0; b < q1; ++b) {
    const chol_gemv_desc d = blocks[b];
    if (d.c_lo >= cw + 16) continue; // the run's rows are zero in the wave's columns
    const TL *A = base + d.a_off + (int64_t)cw * d.lda;
    const double *xs = y + d.x_off;
    for (int r0 = 0; r0 < d.m; r0 += 64 * PER) {
      const int mrows = min(d.m - r0, 64 * PER);
      int ro[PER];
      double xa[PER];
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        ro[u] = r0 + min(lane + 64 * u, mrows - 1);
        xa[u] = (lane + 64 * u < mrows) ? xs[ro[u]] : 0.0;
      }
      TL a[16][PER];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const TL *Ac = A + (int64_t)min(q, ncol - 1) * d.lda;
#pragma unroll
        for (int u = 0; u < PER; ++u) a[q][u] = Ac[ro[u]]; // unconditional (clamped rows repeat the last one, x = 0 there): a predicate here serialises the loads
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
#pragma unroll
        for (int u = 0; u < PER; ++u) acc[q] += (double)a[q][u] * xa[u];
      }
    }
  }
  const double sum = wave_sum16(acc, lane);
  const int c = wave_sum16_col(lane);
  if ((lane & 15) < 4 && c < ncol) unsafeAtomicAdd(&y[blocks[q0].y_off + cw + c], -sum);
}

template <class TL> int chol_launch_solve_dinv(const TL *base, const chol_trsv_desc *descs, int n, int max_n, double *W, hipStream_t st)
{
  if (n <= 0 || max_n <= 0) return 0;
  hipLaunchKernelGGL(k_solve_dinv<TL>, dim3(n, (max_n + TS - 1) / TS), dim3(64), 0, st, base, descs, W);
  return (int)hipGetLastError();
}
#ifndef SOLVE_SPAN32
#define SOLVE_SPAN32 1 /* 0: the fp32 factor's spans through k_solve_trsv<., float> like the fp64 factor's (A/B) */
#endif
// one diagonal span of n separators: different kernels for the fp64 and the fp32 factor (defined with chol_launch_solve_span below, behind the explicit
// instantiations: kernels are emitted in the order of their first use, and the span kernels keep the place they had after every other solve kernel)
static void launch_span(const double *base, const chol_trsv_desc *descs, int n, const double *W, double *y, int col0, bool bwd, hipStream_t st);
static void launch_span(const float *base, const chol_trsv_desc *descs, int n, const double *W, double *y, int col0, bool bwd, hipStream_t st);
#ifndef SOLVE_STEP32
#define SOLVE_STEP32 1 /* 0: span and panel launch by launch at every level (A/B) */
#endif
template <class TL>
static bool launch_steps(const TL *base, const chol_trsv_desc *descs, int n, int max_n, const double *W, double *y, int backward, int *flags, int *gen, const double *W256,
                         double *xt, hipStream_t st)
{ // the few wide separators of a top level: one launch per span step (k_solve_stepw with the spans' explicit inverses, else k_solve_step)
  if (!SOLVE_STEP32 || !flags || n > (W256 ? STEP_MAX_SEPS_W : STEP_MAX_SEPS) || max_n <= SSPAN) return false;
  if (W256) {
    const int nspan = (max_n + SSPAN - 1) / SSPAN;
    for (int i = 0; i < nspan; i++) {
      const int sp = backward ? nspan - 1 - i : i, col0 = sp * SSPAN;
      const int behind = sp > 0 ? max_n - (col0 + SSPAN) : 0;
      const int rows = backward ? SPANEL_BW_ROWS : SPANEL_FW_ROWS;
      const dim3 grid(n, 2 * STEP_NB + (behind > 0 ? 2 * ((behind + rows - 1) / rows) : 0));
      *gen = *gen == 0x7fffffff ? 1 : *gen + 1;
      if (backward) hipLaunchKernelGGL((k_solve_stepw<true, TL>), grid, dim3(256), 0, st, base, descs, W256, nspan, y, xt, col0, flags, *gen);
      else hipLaunchKernelGGL((k_solve_stepw<false, TL>), grid, dim3(256), 0, st, base, descs, W256, nspan, y, xt, col0, flags, *gen);
    }
    return true;
  }
  const int nspan = (max_n + SSPAN - 1) / SSPAN;
  for (int i = 0; i < nspan; i++) {
    const int sp = backward ? nspan - 1 - i : i, col0 = sp * SSPAN;
    const int behind = sp > 0 ? max_n - (col0 + SSPAN) : 0; // rows behind span sp: the previous span's rest
    const int rows = backward ? SPANEL_BW_ROWS : SPANEL_FW_ROWS;
    const int nrest = behind > 0 ? (behind + rows - 1) / rows : 0;
    const bool mid = backward ? sp > 0 : max_n > col0 + SSPAN;
    const dim3 grid(n, nrest > 0 ? 1 + STEP_NB + nrest : mid ? 1 + STEP_NB : 1);
    *gen = *gen == 0x7fffffff ? 1 : *gen + 1;
    if (backward) hipLaunchKernelGGL((k_solve_step<true, TL>), grid, dim3(256), 0, st, base, descs, W, y, col0, flags, *gen);
    else hipLaunchKernelGGL((k_solve_step<false, TL>), grid, dim3(256), 0, st, base, descs, W, y, col0, flags, *gen);
  }
  return true;
}
#ifndef SOLVE_LEAF32
#define SOLVE_LEAF32 1 /* 0: banded leaves span by span, launch by launch (A/B) */
#endif
template <class TL> static bool launch_leaves(const TL *base, const chol_trsv_desc *descs, int n, const double *W, double *y, int backward, hipStream_t st)
{
  if (!SOLVE_LEAF32) return false;
  if (backward) hipLaunchKernelGGL((k_solve_leaf32<true, TL>), dim3(n), dim3(256), 0, st, base, descs, W, y);
  else hipLaunchKernelGGL((k_solve_leaf32<false, TL>), dim3(n), dim3(256), 0, st, base, descs, W, y);
  return true;
}
template <class TL>
int chol_launch_solve_trsv(const TL *base, const chol_trsv_desc *descs, int n, int max_n, int max_under, const double *W, double *y, int backward, int *flags, int *gen,
                           const double *W256, double *xt, hipStream_t st)
{ // all separators of a level; wide ones in spans of SSPAN columns: diagonal span by one workgroup each, the rows below by all CUs (max_under: the most
  // rows any separator of the level has to read under a span -- its band if it is a leaf; negative: every separator of the level is banded within one span)
  if (n <= 0) return 0;
  if (max_under < 0) {
    if (max_n > SSPAN && launch_leaves(base, descs, n, W, y, backward, st)) return (int)hipGetLastError();
    max_under = -max_under;
  }
  if (launch_steps(base, descs, n, max_n, W, y, backward, flags, gen, W256, xt, st)) return (int)hipGetLastError();
  const int nspan = (max_n + SSPAN - 1) / SSPAN;
  for (int i = 0; i < nspan; i++) {
    const int sp = backward ? nspan - 1 - i : i, col0 = sp * SSPAN;
    const int below = min(max_n - (col0 + SSPAN), max_under); // rows under the span in the widest separator
    if (backward) {
      if (below > 0) hipLaunchKernelGGL((k_solve_panel<true, TL>), dim3(n, (below + SPANEL_BW_ROWS - 1) / SPANEL_BW_ROWS), dim3(256), 0, st, base, descs, y, col0);
      launch_span(base, descs, n, W, y, col0, true, st);
    } else {
      launch_span(base, descs, n, W, y, col0, false, st);
      if (below > 0) hipLaunchKernelGGL((k_solve_panel<false, TL>), dim3(n, (below + 255) / 256), dim3(256), 0, st, base, descs, y, col0);
    }
  }
  return (int)hipGetLastError();
}
template <class TL> int chol_launch_solve_inv256(const TL *base, const chol_trsv_desc *descs, int n, int max_n, const double *W16, double *W256, hipStream_t st)
{
  if (n <= 0 || max_n <= SSPAN) return 0;
  const int nspan = (max_n + SSPAN - 1) / SSPAN;
  hipLaunchKernelGGL(k_solve_inv256<TL>, dim3(n, nspan, SSPAN / TS), dim3(64), 0, st, base, descs, W16, W256, nspan);
  return (int)hipGetLastError();
}
template <class TL> int chol_launch_solve_offdiag(const TL *base, const chol_gemv_desc *blocks, const int *items, int n_items, double *y, int backward, hipStream_t st)
{
  if (n_items <= 0) return 0;
  if (backward) hipLaunchKernelGGL(k_solve_gather_bwd<TL>, dim3(n_items), dim3(256), 0, st, base, blocks, items, y);
  else hipLaunchKernelGGL(k_solve_gemv_fwd<TL>, dim3(n_items), dim3(256), 0, st, base, blocks, items, y);
  return (int)hipGetLastError();
}
int chol_launch_permute(const double *in, const int *perm, double *out, int n, int inverse, hipStream_t st)
{
  if (n <= 0) return 0;
  if (inverse) hipLaunchKernelGGL(k_permute_out, dim3((n + 255) / 256), dim3(256), 0, st, in, perm, out, n);
  else hipLaunchKernelGGL(k_permute_in, dim3((n + 255) / 256), dim3(256), 0, st, in, perm, out, n);
  return (int)hipGetLastError();
}
template int chol_launch_solve_dinv(const double *, const chol_trsv_desc *, int, int, double *, hipStream_t);
template int chol_launch_solve_trsv(const double *, const chol_trsv_desc *, int, int, int, const double *, double *, int, int *, int *, const double *, double *, hipStream_t);
template int chol_launch_solve_inv256(const double *, const chol_trsv_desc *, int, int, const double *, double *, hipStream_t);
template int chol_launch_solve_inv256(const float *, const chol_trsv_desc *, int, int, const double *, double *, hipStream_t);
template int chol_launch_solve_offdiag(const double *, const chol_gemv_desc *, const int *, int, double *, int, hipStream_t);
template int chol_launch_solve_dinv(const float *, const chol_trsv_desc *, int, int, double *, hipStream_t);
template int chol_launch_solve_trsv(const float *, const chol_trsv_desc *, int, int, int, const double *, double *, int, int *, int *, const double *, double *, hipStream_t);
template int chol_launch_solve_offdiag(const float *, const chol_gemv_desc *, const int *, int, double *, int, hipStream_t);
static void launch_span(const double *base, const chol_trsv_desc *descs, int n, const double *W, double *y, int col0, bool bwd, hipStream_t st)
{
  if (bwd) hipLaunchKernelGGL((k_solve_trsv<true, double>), dim3(n), dim3(256), 0, st, base, descs, W, y, col0);
  else hipLaunchKernelGGL((k_solve_trsv<false, double>), dim3(n), dim3(256), 0, st, base, descs, W, y, col0);
}
template <bool BWD> static void launch_span32(const float *base, const chol_trsv_desc *descs, int n, const double *W, double *y, int col0, hipStream_t st)
{
  if (SOLVE_SPAN32) hipLaunchKernelGGL((k_solve_span32<BWD>), dim3(n), dim3(256), 0, st, base, descs, W, y, col0);
  else hipLaunchKernelGGL((k_solve_trsv<BWD, float>), dim3(n), dim3(256), 0, st, base, descs, W, y, col0);
}
static void launch_span(const float *base, const chol_trsv_desc *descs, int n, const double *W, double *y, int col0, bool bwd, hipStream_t st)
{
  if (bwd) launch_span32<true>(base, descs, n, W, y, col0, st); else launch_span32<false>(base, descs, n, W, y, col0, st);
}
// one 256-column diagonal span of every separator of a level on its own (plain stores; the deterministic solve puts its gathers between them)
template <class TL> int chol_launch_solve_span(const TL *base, const chol_trsv_desc *descs, int n, const double *W, double *y, int col0, int backward, hipStream_t st)
{
  if (n <= 0) return 0;
  launch_span(base, descs, n, W, y, col0, backward != 0, st);
  return (int)hipGetLastError();
}
template int chol_launch_solve_span(const double *, const chol_trsv_desc *, int, const double *, double *, int, int, hipStream_t);
template int chol_launch_solve_span(const float *, const chol_trsv_desc *, int, const double *, double *, int, int, hipStream_t);
int chol_launch_trsv_fwd(const double *base, const chol_trsv_desc *descs, int n, double *y, hipStream_t st)
{
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_trsv_fwd, dim3(n), dim3(256), 0, st, base, descs, y);
  return (int)hipGetLastError();
}
int chol_launch_gemv_fwd(const double *base, const chol_gemv_desc *descs, const int *grp_start, const int *grp_rows, int ngroups, double *y, hipStream_t st)
{
  if (ngroups <= 0) return 0;
  hipLaunchKernelGGL(k_gemv_fwd, dim3(ngroups), dim3(256), 0, st, base, descs, grp_start, grp_rows, y);
  return (int)hipGetLastError();
}
int chol_launch_bwd(const double *base, const chol_trsv_desc *descs, const chol_gemv_desc *gd, const int *gstart, int n, double *y, hipStream_t st)
{
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_bwd, dim3(n), dim3(256), 0, st, base, descs, gd, gstart, y);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Iterative refinement helpers (fp64): r = b - A x with A as a symmetric CSR in original dof order, per-workgroup
// partial sums of r^2 and b^2 (added on the host: deterministic), x += dx.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_residual_csr(const int64_t *__restrict__ ptr, const int *__restrict__ col, const double *__restrict__ val,
                                                      const double *__restrict__ b, const double *__restrict__ x, double *__restrict__ r, int n, double *__restrict__ partial)
{
  __shared__ double s2[2][4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double ri = 0.0, bi = 0.0;
  if (i < n) {
    bi = b[i];
    double acc = bi;
    for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) acc = fma(-val[e], x[col[e]], acc);
    ri = acc;
    if (r) r[i] = ri;
  }
  double a = ri * ri, c = bi * bi;
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); c += __shfl_down(c, o, 64); }
  if ((threadIdx.x & 63) == 0) { s2[0][threadIdx.x >> 6] = a; s2[1][threadIdx.x >> 6] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = ((s2[0][0] + s2[0][1]) + s2[0][2]) + s2[0][3];
    partial[2 * blockIdx.x + 1] = ((s2[1][0] + s2[1][1]) + s2[1][2]) + s2[1][3];
  }
}
__global__ void k_axpy1(double *__restrict__ x, const double *__restrict__ dx, int n)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] += dx[i];
}
int chol_launch_residual(const int64_t *ptr, const int *col, const double *val, const double *b, const double *x, double *r, int n, double *partial, hipStream_t st)
{
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_residual_csr, dim3((n + 255) / 256), dim3(256), 0, st, ptr, col, val, b, x, r, n, partial);
  return (int)hipGetLastError();
}
int chol_launch_axpy1(double *x, const double *dx, int n, hipStream_t st)
{
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_axpy1, dim3((n + 255) / 256), dim3(256), 0, st, x, dx, n);
  return (int)hipGetLastError();
}
