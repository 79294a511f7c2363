// Block form of the forward products: Y = L Z and Y = L^T Z in permuted coordinates for a chunk of CHOL_NRHS_W = 32 columns (cholamd_multiply_half_nrhs /
// cholamd_multiply_nrhs and their _f32 forms).  The work list is that of the single-vector products (chol_mul_lists: one workgroup per ITEM, an item owns
// 16 consecutive positions of the result and walks its sources in list order), the arithmetic that of the block solve: a tile of 16 lines x 32 columns on
// v_mfma_f64_16x16x4_f64, two accumulators per wave, so every stored entry of L is read once per chunk and carries 64 flops instead of 2.
//
// The chunk's input is the permuted block Zp (n x 32, ROW-major: the 32 values of one permuted row are 256 contiguous bytes; k_nrhs_permute_in of
// chol_solve_nrhs.hip writes it, padding columns zero).  The four waves of a workgroup share every source: its reduction range is cut into chunks of
// CHOL_MULN_KSTEP = 32 steps which go round robin over the waves (chol_muln_wave, chol_plan.h); a wave keeps ONE partial tile over all sources, the four
// tiles are added in wave order out of LDS.  One owner per element, a fixed order, no floating-point atomics: two calls return the same bits.
//
// Operands (v_mfma_f64_16x16x4_f64: lane l holds A(l & 15, k = l >> 4) and B(k = l >> 4, l & 15); result register q: line (l >> 4) + 4 q, column l & 15):
//   FORWARD   A(i, k) = L[a_off + i + k ld]: the 16 lanes of a step run along a column of the panel, one 128-byte segment (64 of an fp32 factor)
//   BACKWARD  A(j, k) = L[a_off + k + j ld]: a lane reads 8 bytes of column j; the four lane groups of a step read 4 consecutive rows (32 bytes), the 8
//             steps of a chunk the 32 consecutive rows of the chunk: 16 columns x 256 contiguous bytes per wave and chunk, every 128-byte line fetched
//             from HBM once and used whole by back-to-back loads of the same wave (DESIGN.md section 13 at "BACKWARD operand")
//   B(k, j) = Zp[(z_off + k) 32 + j]: 16 lanes read 128 contiguous bytes
// An operand that is not meant -- above the diagonal of a diagonal block, a line >= nv, a step >= len -- is read clamped inside the strip and SELECTED to
// 0.0 (chol_muln_elem); the upper triangles may hold NaN.  B is selected to 0.0 for steps >= len too.  Everything after the load is fp64.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chol_kernels.h"
#include "chol_plan.h"

#define NW CHOL_NRHS_W
#define MULN_THREADS (64 * CHOL_MULN_WAVES)
#define MULN_U (CHOL_MULN_KSTEP / 4) // MFMA steps per chunk
#define MULN_RED_LD (NW + 1)         // partial tiles in LDS, rows padded: the lane groups of a result register are 4 lines apart
static_assert(NW == 32 && CHOL_MUL_TILE == 16 && CHOL_MULN_WAVES == 4, "a tile is 16 lines x two 16-column halves, four waves per item");

typedef double nd4 __attribute__((ext_vector_type(4)));

template <class TL, int BW>
__global__ __launch_bounds__(MULN_THREADS) void k_multiply_nrhs(const TL *__restrict__ base, const chol_mul_item *__restrict__ items, const chol_mul_src *__restrict__ srcs,
                                                                const double *__restrict__ Zp, double *__restrict__ Y, const int *__restrict__ perm, int64_t ldy, int c0, int cols)
{
  __shared__ double red[CHOL_MULN_WAVES * CHOL_MUL_TILE * MULN_RED_LD];
  const chol_mul_item it = items[blockIdx.x];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i16 = lane & 15, g = lane >> 4;
  nd4 acc0 = { 0.0, 0.0, 0.0, 0.0 }, acc1 = { 0.0, 0.0, 0.0, 0.0 };
  for (int s = it.src_first; s < it.src_end; s++) {
    const chol_mul_src q = srcs[s];
    const double *__restrict__ B = Zp + (int64_t)q.z_off * NW;
    // this wave's chunks of the source: c = first, first + 4, ... with chol_muln_wave(s - src_first, c) == wave
    const int first = (wave - (s - it.src_first)) & (CHOL_MULN_WAVES - 1);
    for (int k0 = first * CHOL_MULN_KSTEP; k0 < q.len; k0 += CHOL_MULN_WAVES * CHOL_MULN_KSTEP) {
      double a[MULN_U], b0[MULN_U], b1[MULN_U];
#pragma unroll
      for (int u = 0; u < MULN_U; ++u) {
        const int k = k0 + 4 * u + g, kk = min(k, q.len - 1);
        int meant;
        const int64_t e = chol_muln_elem(&q, BW, it.nv, i16, k, &meant);
        const double v = (double)base[e];
        a[u] = meant ? v : 0.0;
        const double z0 = B[(int64_t)kk * NW + i16], z1 = B[(int64_t)kk * NW + 16 + i16];
        b0[u] = k < q.len ? z0 : 0.0;
        b1[u] = k < q.len ? z1 : 0.0;
      }
#pragma unroll
      for (int u = 0; u < MULN_U; ++u) {
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b0[u], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b1[u], acc1, 0, 0, 0);
      }
    }
  }
  double *mine = red + wave * (CHOL_MUL_TILE * MULN_RED_LD);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mine[(g + 4 * r) * MULN_RED_LD + i16] = acc0[r];
    mine[(g + 4 * r) * MULN_RED_LD + 16 + i16] = acc1[r];
  }
  __syncthreads();
  // 512 results, two per lane, the waves' partial tiles in wave order
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int e = t + h * MULN_THREADS;
    // the last stage of a call (perm): consecutive lanes along the lines of one column of Y; a first stage: along the 32 columns of a row of the block
    const int line = perm ? (e & (CHOL_MUL_TILE - 1)) : e / NW, j = perm ? e / CHOL_MUL_TILE : (e & (NW - 1));
    double sum = red[line * MULN_RED_LD + j];
#pragma unroll
    for (int w = 1; w < CHOL_MULN_WAVES; ++w) sum += red[w * (CHOL_MUL_TILE * MULN_RED_LD) + line * MULN_RED_LD + j];
    if (line < it.nv) {
      const int pos = it.y_off + line;
      if (perm) { if (j < cols) Y[perm[pos] + (int64_t)(c0 + j) * ldy] = sum; }
      else Y[(int64_t)pos * NW + j] = sum;
    }
  }
}

template <class TL>
int chol_launch_multiply_nrhs(const TL *base, const chol_mul_item *items, int n_items, const chol_mul_src *srcs, int backward, const double *Zp, double *Y, const int *perm,
                              int64_t ldy, int c0, int cols, hipStream_t st)
{
  if (n_items <= 0) return 0;
  if (backward) hipLaunchKernelGGL((k_multiply_nrhs<TL, 1>), dim3(n_items), dim3(MULN_THREADS), 0, st, base, items, srcs, Zp, Y, perm, ldy, c0, cols);
  else hipLaunchKernelGGL((k_multiply_nrhs<TL, 0>), dim3(n_items), dim3(MULN_THREADS), 0, st, base, items, srcs, Zp, Y, perm, ldy, c0, cols);
  return (int)hipGetLastError();
}

template int chol_launch_multiply_nrhs(const double *, const chol_mul_item *, int, const chol_mul_src *, int, const double *, double *, const int *, int64_t, int, int, hipStream_t);
template int chol_launch_multiply_nrhs(const float *, const chol_mul_item *, int, const chol_mul_src *, int, const double *, double *, const int *, int64_t, int, int, hipStream_t);
