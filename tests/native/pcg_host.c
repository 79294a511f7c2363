/* cholamd_plan_apply_host (y = A x in the device's fma order: the host side of cholamd_apply and of the PCG loop's operator) under the sanitizers, without
 * an interpreter in the process: `make pcg_host` builds this against the sanitizer build and runs it with LeakSanitizer on.  It generates its own inputs
 * (Laplacians whose row counts sit around the 256-row workgroups of the device kernel), calls with exact-size buffers (an access past them is the
 * sanitizer's to report), checks the product against the stencil written out by hand, the value-array form against the plan's own values, and the
 * refusals.  No GPU call. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "cholamd.h"

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

static int run(int nx, int ny, int nz, int levels)
{
  cholamd_problem *g = NULL;
  cholamd_plan *p = NULL;
  if (cholamd_generate_laplacian(nx, ny, nz, levels, 16, &g) || cholamd_plan_create_from_problem(g, &p)) FAIL("generate %d x %d x %d: %s", nx, ny, nz, cholamd_last_error());
  const int n = cholamd_plan_n(p), nzf = cholamd_plan_nz(p);
  if (n != nx * ny * nz) FAIL("n = %d", n);
  double *x = malloc((size_t)n * sizeof(double)), *y = malloc((size_t)n * sizeof(double)), *y2 = malloc((size_t)n * sizeof(double));
  double *v = malloc((size_t)nzf * sizeof(double));
  int *row = malloc((size_t)nzf * sizeof(int)), *col = malloc((size_t)nzf * sizeof(int));
  if (!x || !y || !y2 || !v || !row || !col) FAIL("out of memory");
  for (int i = 0; i < n; i++) x[i] = sin(0.37 * (i + 1)) + 0.01 * (i % 7);
  if (cholamd_plan_entries(p, row, col)) FAIL("entries: %s", cholamd_last_error());
  const double diag = 2.0 * ((nx > 1) + (ny > 1) + (nz > 1));
  for (int k = 0; k < nzf; k++) v[k] = row[k] == col[k] ? diag : -1.0; /* the generator's Laplacian as a value array */
  if (cholamd_plan_apply_host(p, NULL, x, y) || cholamd_plan_apply_host(p, v, x, y2)) FAIL("apply: %s", cholamd_last_error());
  if (memcmp(y, y2, (size_t)n * sizeof(double))) FAIL("%d x %d x %d: the value-array form differs from the plan's own values", nx, ny, nz);
  for (int z = 0; z < nz; z++)
    for (int yy = 0; yy < ny; yy++)
      for (int xx = 0; xx < nx; xx++) {
        const int j = xx + nx * (yy + ny * z);
        double ref = diag * x[j], mag = fabs(diag * x[j]);
        const int nb[6] = { xx > 0 ? j - 1 : -1, xx + 1 < nx ? j + 1 : -1, yy > 0 ? j - nx : -1, yy + 1 < ny ? j + nx : -1, z > 0 ? j - nx * ny : -1, z + 1 < nz ? j + nx * ny : -1 };
        for (int q = 0; q < 6; q++) if (nb[q] >= 0) { ref -= x[nb[q]]; mag += fabs(x[nb[q]]); }
        if (!(fabs(y[j] - ref) <= 8.0 * 1.1102230246251565e-16 * mag)) FAIL("%d x %d x %d: y[%d] = %.17g, stencil %.17g", nx, ny, nz, j, y[j], ref);
      }
  for (int k = 0; k < nzf; k++) v[k] *= 1.0 + 0.25 * (k % 3); /* other values: linear in the value array */
  if (cholamd_plan_apply_host(p, v, x, y2)) FAIL("apply: %s", cholamd_last_error());
  int same = 1;
  for (int i = 0; i < n; i++) same &= y[i] == y2[i];
  if (same && n > 1) FAIL("new values changed nothing");
  /* refusals: nothing written */
  for (int i = 0; i < n; i++) y[i] = 7.0;
  if (cholamd_plan_apply_host(p, NULL, NULL, y) != CHOLAMD_ERR_ARG || cholamd_plan_apply_host(p, NULL, x, NULL) != CHOLAMD_ERR_ARG ||
      cholamd_plan_apply_host(NULL, NULL, x, y) != CHOLAMD_ERR_ARG || cholamd_plan_apply_host(p, NULL, y, y) != CHOLAMD_ERR_ARG) FAIL("a bad call was not refused");
  for (int i = 0; i < n; i++) if (y[i] != 7.0) FAIL("a refused call wrote y[%d]", i);
  free(x); free(y); free(y2); free(v); free(row); free(col);
  cholamd_plan_destroy(p);
  cholamd_problem_destroy(g);
  return 0;
}

int main(void)
{
  const int sizes[][4] = { { 3, 3, 1, 2 }, { 5, 5, 1, 3 }, { 16, 16, 1, 3 }, { 17, 15, 1, 3 }, { 20, 20, 1, 3 }, { 7, 5, 3, 3 }, { 15, 15, 15, 5 } };
  for (size_t q = 0; q < sizeof sizes / sizeof *sizes; q++)
    if (run(sizes[q][0], sizes[q][1], sizes[q][2], sizes[q][3])) return 1;
  printf("pcg_host: ok\n");
  return 0;
}
