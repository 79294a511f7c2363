/* Host restatements of the low-rank kernels' partition (include/cholamd.h at cholamd_lowrank_slabs; chol_plan.h at CHOL_LR_SLAB): no device.  They walk
 * the slabs, stage blocks, 4-row MFMA steps and 16-row chunks of chol_lowrank.hip in its order, so a test of them is a test of the kernels' index logic;
 * the bits are not the device's (an MFMA step adds its four products in an order of its own). */
#include <stddef.h>
#include <stdint.h>

#include "chol_plan.h"
#include "cholamd.h"

_Static_assert(CHOLAMD_LOWRANK_MAX == CHOL_LR_MAX, "the public limit is the kernels' limit");

int cholamd_lowrank_slabs(int64_t n, int64_t *first_row, int64_t cap)
{
  if (n < 0 || (first_row && cap < 0)) { chol_set_error("cholamd_lowrank_slabs: n = %lld, cap = %lld", (long long)n, (long long)cap); return CHOLAMD_ERR_ARG; }
  const int64_t ns = chol_lr_slabs(n);
  if (ns > INT32_MAX) { chol_set_error("cholamd_lowrank_slabs: %lld slabs", (long long)ns); return CHOLAMD_ERR_ARG; }
  if (first_row) for (int64_t s = 0; s < ns && s < cap; s++) first_row[s] = s * CHOL_LR_SLAB;
  return (int)ns;
}

static int lr_host_args(const char *what, int64_t n, int k, int m, const void *a, int64_t lda, int64_t amin, const void *b, int64_t ldb, int64_t bmin, const void *c, int64_t ldc, int64_t cmin)
{ /* 1: nothing to do */
  if (n < 0 || k < 0 || m < 0 || k > CHOL_LR_MAX) { chol_set_error("%s: n = %lld, k = %d, m = %d (k at most %d)", what, (long long)n, k, m, CHOL_LR_MAX); return CHOLAMD_ERR_ARG; }
  if (lda < amin || ldb < bmin || ldc < cmin || lda < 1 || ldb < 1 || ldc < 1) {
    chol_set_error("%s: leading dimensions %lld, %lld, %lld must be at least %lld, %lld, %lld", what, (long long)lda, (long long)ldb, (long long)ldc, (long long)amin, (long long)bmin, (long long)cmin);
    return CHOLAMD_ERR_ARG;
  }
  if (k == 0 || m == 0) return 1;
  if (!c || (n > 0 && (!a || !b))) { chol_set_error("%s: NULL pointer", what); return CHOLAMD_ERR_ARG; }
  return 0;
}

int cholamd_lowrank_tprod_host(int64_t n, int k, int m, const double *P, int64_t ldp, const double *Q, int64_t ldq, double *T, int64_t ldt)
{
  int rc = lr_host_args("cholamd_lowrank_tprod_host", n, k, m, P, ldp, n, Q, ldq, n, T, ldt, k);
  if (rc) return rc > 0 ? 0 : rc;
  const int64_t ns = chol_lr_slabs(n);
  for (int j = 0; j < m; j++)
    for (int i = 0; i < k; i++) {
      const double *p = P + (int64_t)i * ldp, *q = Q + (int64_t)j * ldq;
      double sum = 0.0;
      for (int64_t s = 0; s < ns; s++) { /* the slab's partial: stage blocks of CHOL_LR_STAGE rows, steps of 4 rows, rows >= n selected away */
        const int64_t r1 = (s + 1) * CHOL_LR_SLAB < n ? (s + 1) * CHOL_LR_SLAB : n;
        double part = 0.0;
        for (int64_t r0 = s * CHOL_LR_SLAB; r0 < r1; r0 += CHOL_LR_STAGE)
          for (int u = 0; u < CHOL_LR_STAGE; u += 4) {
            double step = 0.0;
            for (int g = 0; g < 4; g++) { const int64_t r = r0 + u + g; step += r < r1 ? p[r] * q[r] : 0.0; }
            part += step;
          }
        sum = s ? sum + part : part;
      }
      T[i + (int64_t)j * ldt] = sum; /* n == 0: no slab, 0.0 */
    }
  return 0;
}

int cholamd_lowrank_rprod_host(int64_t n, int k, int m, double alpha, double beta, const double *V, int64_t ldv, const double *T, int64_t ldt, double *X, int64_t ldx)
{
  int rc = lr_host_args("cholamd_lowrank_rprod_host", n, k, m, V, ldv, n, T, ldt, k, X, ldx, n);
  if (rc) return rc > 0 ? 0 : rc;
  /* a call of at most 32 columns: the reduction is shared by CHOL_LR_RWAVES waves (k_lr_rprod32); else one wave owns it */
  const int steps = (k + 3) / 4, waves = m <= 32 ? CHOL_LR_RWAVES : 1, sw = (steps + waves - 1) / waves;
  double vrow[CHOL_LR_ROWS][CHOL_LR_MAX];
  for (int64_t r0 = 0; r0 < n; r0 += CHOL_LR_ROWS) { /* a chunk's rows of V are read whole before its first store: X == V with m == k is legal */
    const int rows = n - r0 < CHOL_LR_ROWS ? (int)(n - r0) : CHOL_LR_ROWS;
    for (int c = 0; c < k; c++) for (int r = 0; r < rows; r++) vrow[r][c] = V[r0 + r + (int64_t)c * ldv];
    for (int j = 0; j < m; j++)
      for (int r = 0; r < rows; r++) {
        double acc = 0.0;
        for (int w = 0; w < waves; w++) { /* a wave's range of 4-column steps; the ranges' partial sums in wave order */
          double part = 0.0;
          for (int s = w * sw; s < (w + 1) * sw && s < steps; s++) {
            double step = 0.0;
            for (int c = 4 * s; c < 4 * s + 4 && c < k; c++) step += T[c + (int64_t)j * ldt] * vrow[r][c];
            part += step;
          }
          acc = w ? acc + part : part;
        }
        double *x = X + r0 + r + (int64_t)j * ldx;
        *x = alpha != 0.0 ? alpha * *x + beta * acc : beta * acc;
      }
  }
  return 0;
}
