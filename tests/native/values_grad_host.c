/* The host restatements of the values-gradient kernels (cholamd_plan_values_grad_pairs_host, cholamd_plan_values_grad_logdet_host,
 * cholamd_plan_duplicate_entries) under the sanitizers, without an interpreter in the process: `make values_grad_host` builds this against the sanitizer
 * build and runs it with LeakSanitizer on.  Generated Laplacians, exact-size buffers (an access past them is the sanitizer's to report), the pair sums
 * against plain long-double loops within the inner-product bound, alpha / beta, P == Q, the log-det walk over an arena filled from a known value array
 * (it must return m_k v_k exactly), and the refusals.  No GPU call. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "cholamd.h"

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)
static const double U = 1.1102230246251565e-16; /* 2^-53 */

static double *gen(int64_t count, double f)
{
  double *v = malloc((size_t)(count > 0 ? count : 1) * sizeof(double));
  if (v) for (int64_t i = 0; i < count; i++) v[i] = sin(f * (double)(i + 1)) + 0.01 * (double)(i % 7);
  return v;
}

static int run_pairs(const cholamd_plan *p, const int *row, const int *col, int nrhs, int64_t ldp, int64_t ldq, int same)
{
  const int n = cholamd_plan_n(p), nz = cholamd_plan_nz(p);
  const int64_t np = (int64_t)(nrhs - 1) * ldp + n, nq = (int64_t)(nrhs - 1) * ldq + n; /* the full extents, not ld * nrhs */
  double *P = gen(np, 0.37), *Q = same ? P : gen(nq, 0.11), *g = malloc((size_t)nz * sizeof(double)), *g2 = malloc((size_t)nz * sizeof(double));
  if (!P || !Q || !g || !g2) FAIL("out of memory");
  if (same) ldq = ldp;
  for (int k = 0; k < nz; k++) g[k] = NAN;
  if (cholamd_plan_values_grad_pairs_host(p, P, ldp, Q, ldq, nrhs, 1.0, 0.0, g, nz)) FAIL("pairs: %s", cholamd_last_error());
  for (int k = 0; k < nz; k++) {
    const int64_t i = row[k], j = col[k];
    long double ref = 0.0L, mag = 0.0L;
    for (int c = 0; c < nrhs; c++) {
      ref += (long double)P[i + c * ldp] * Q[j + c * ldq]; mag += fabsl((long double)P[i + c * ldp] * Q[j + c * ldq]);
      if (i != j) { ref += (long double)P[j + c * ldp] * Q[i + c * ldq]; mag += fabsl((long double)P[j + c * ldp] * Q[i + c * ldq]); }
    }
    if (!(fabsl((long double)g[k] - ref) <= (2.0L * nrhs + 1.0L) * U * mag)) FAIL("pairs nrhs = %d: g[%d] = %.17g, long double loop %.17Lg", nrhs, k, g[k], ref);
  }
  /* alpha = 0.5, beta = 2 accumulates onto what is there */
  for (int k = 0; k < nz; k++) g2[k] = 1.0 + 0.25 * k;
  if (cholamd_plan_values_grad_pairs_host(p, P, ldp, Q, ldq, nrhs, 0.5, 2.0, g2, nz)) FAIL("pairs: %s", cholamd_last_error());
  for (int k = 0; k < nz; k++)
    if (g2[k] != fma(0.5, g[k], 2.0 * (1.0 + 0.25 * k))) FAIL("alpha = 0.5, beta = 2: g[%d] = %.17g", k, g2[k]);
  if (!same) free(Q);
  free(P); free(g); free(g2);
  return 0;
}

static int run_plan(const cholamd_plan *p)
{
  const int n = cholamd_plan_n(p), nz = cholamd_plan_nz(p);
  const int64_t na = cholamd_plan_arena_doubles(p);
  if (cholamd_plan_duplicate_entries(p) != 0 || cholamd_plan_dropped_entries(p) != 0) FAIL("a generated Laplacian has duplicate or dropped entries");
  int *row = malloc((size_t)nz * sizeof(int)), *col = malloc((size_t)nz * sizeof(int));
  if (!row || !col) FAIL("out of memory");
  if (cholamd_plan_entries(p, row, col)) FAIL("entries: %s", cholamd_last_error());
  const int ks[] = { 1, 2, 31, 32, 33, 70 };
  for (size_t q = 0; q < sizeof ks / sizeof *ks; q++)
    if (run_pairs(p, row, col, ks[q], n, n, 0) || run_pairs(p, row, col, ks[q], n + 3, n + 5, 0) || run_pairs(p, row, col, ks[q], n + 1, n + 1, 1)) return 1;
  /* log det: an arena filled from a known value array returns m_k v_k */
  double *vals = gen(nz, 0.19), *arena = malloc((size_t)na * sizeof(double)), *g = malloc((size_t)nz * sizeof(double));
  if (!vals || !arena || !g) FAIL("out of memory");
  for (int k = 0; k < nz; k++) { vals[k] += 2.0; g[k] = NAN; } /* no zero among them */
  if (cholamd_plan_fill_host_values(p, vals, nz, arena)) FAIL("fill: %s", cholamd_last_error());
  if (cholamd_plan_values_grad_logdet_host(p, arena, 1.0, 0.0, g, nz)) FAIL("logdet: %s", cholamd_last_error());
  for (int k = 0; k < nz; k++) if (g[k] != (row[k] == col[k] ? 1.0 : 2.0) * vals[k]) FAIL("logdet: g[%d] = %.17g, value %.17g", k, g[k], vals[k]);
  if (cholamd_plan_values_grad_logdet_host(p, arena, -0.5, 3.0, g, nz)) FAIL("logdet: %s", cholamd_last_error());
  for (int k = 0; k < nz; k++) {
    const double t = (row[k] == col[k] ? 1.0 : 2.0) * vals[k];
    if (g[k] != fma(-0.5, t, 3.0 * t)) FAIL("logdet alpha = -0.5, beta = 3: g[%d] = %.17g", k, g[k]);
  }
  /* the refusals write nothing; nrhs == 0 touches nothing */
  double *P = gen((int64_t)n * 2, 0.3);
  if (!P) FAIL("out of memory");
  for (int k = 0; k < nz; k++) g[k] = -7.0;
  if (cholamd_plan_values_grad_pairs_host(p, P, n, P, n, 2, 1.0, 0.0, g, nz - 1) != CHOLAMD_ERR_ARG ||
      cholamd_plan_values_grad_pairs_host(p, P, n, P, n, 2, 1.0, 0.0, g, nz + 1) != CHOLAMD_ERR_ARG ||
      cholamd_plan_values_grad_pairs_host(p, P, n - 1, P, n, 2, 1.0, 0.0, g, nz) != CHOLAMD_ERR_ARG ||
      cholamd_plan_values_grad_pairs_host(p, P, n, P, n - 1, 2, 1.0, 0.0, g, nz) != CHOLAMD_ERR_ARG ||
      cholamd_plan_values_grad_pairs_host(p, P, n, P, n, -1, 1.0, 0.0, g, nz) != CHOLAMD_ERR_ARG ||
      cholamd_plan_values_grad_pairs_host(p, NULL, n, P, n, 2, 1.0, 0.0, g, nz) != CHOLAMD_ERR_ARG ||
      cholamd_plan_values_grad_pairs_host(p, P, n, NULL, n, 2, 1.0, 0.0, g, nz) != CHOLAMD_ERR_ARG ||
      cholamd_plan_values_grad_pairs_host(p, P, n, P, n, 2, 1.0, 0.0, NULL, nz) != CHOLAMD_ERR_ARG ||
      cholamd_plan_values_grad_pairs_host(NULL, P, n, P, n, 2, 1.0, 0.0, g, nz) != CHOLAMD_ERR_ARG ||
      cholamd_plan_values_grad_logdet_host(p, arena, 1.0, 0.0, g, nz + 1) != CHOLAMD_ERR_ARG ||
      cholamd_plan_values_grad_logdet_host(p, NULL, 1.0, 0.0, g, nz) != CHOLAMD_ERR_ARG ||
      cholamd_plan_values_grad_logdet_host(p, arena, 1.0, 0.0, NULL, nz) != CHOLAMD_ERR_ARG ||
      cholamd_plan_values_grad_logdet_host(NULL, arena, 1.0, 0.0, g, nz) != CHOLAMD_ERR_ARG)
    FAIL("a bad argument is accepted");
  if (cholamd_plan_values_grad_pairs_host(p, NULL, n, NULL, n, 0, 1.0, 0.0, NULL, nz)) FAIL("nrhs = 0 is refused");
  for (int k = 0; k < nz; k++) if (g[k] != -7.0) FAIL("a refused call wrote g");
  free(P); free(vals); free(arena); free(g); free(row); free(col);
  return 0;
}

int main(void)
{
  const int grids[][5] = { { 7, 5, 3, 3, 4 }, { 12, 12, 12, 4, 16 }, { 20, 20, 1, 3, 16 } };
  for (size_t q = 0; q < sizeof grids / sizeof *grids; q++) {
    cholamd_problem *g = NULL;
    if (cholamd_generate_laplacian(grids[q][0], grids[q][1], grids[q][2], grids[q][3], grids[q][4], &g)) { fprintf(stderr, "generate: %s\n", cholamd_last_error()); return 1; }
    cholamd_plan *p = NULL;
    if (cholamd_plan_create_from_problem(g, &p)) { fprintf(stderr, "problem plan: %s\n", cholamd_last_error()); return 1; }
    if (run_plan(p)) return 1;
    cholamd_plan_destroy(p);
    cholamd_problem_destroy(g);
  }
  printf("values_grad_host: ok\n");
  return 0;
}
