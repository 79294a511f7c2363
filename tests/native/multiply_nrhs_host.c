/* The host restatement of the block products with the factor (cholamd_plan_multiply_host_nrhs) under the sanitizers, without an interpreter in the
 * process: `make asan` builds this against the sanitizer build and runs it with LeakSanitizer on.  The walk uses the block kernel's own index logic
 * (chol_plan.h: chol_muln_wave, chol_muln_elem -- it reads every operand of a 16 x 32-step chunk CLAMPED into the strip, meant or not), so an arena of
 * exactly cholamd_plan_arena_doubles elements makes a clamp that leaves the strip the sanitizer's to report.  Plans of the fixtures and of a generated grid,
 * exact-size buffers, 1, 32 and 33 columns, both directions and the full product, in place, the refusals.  The arena is the plain host fill: tril(P A P^T)
 * stands in for L (it lies inside the envelope the leaf skips assume), so a half product is checked against the dense image of the arena with the
 * inner-product bound (k + 2) u |L| |z|, k <= n, and the full product against the FORWARD product of the BACKWARD product, bit for bit.  No GPU call is made. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "cholamd.h"

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

static int run_plan(cholamd_plan *p)
{
  static const int counts[3] = { 1, 32, 33 };
  const int n = cholamd_plan_n(p), K = 33;
  const int64_t na = cholamd_plan_arena_doubles(p);
  const size_t blk = (size_t)n * K;
  double *arena = malloc((size_t)na * sizeof(double)), *dense = malloc((size_t)n * n * sizeof(double));
  double *Z = malloc(blk * sizeof(double)), *Y = malloc(blk * sizeof(double)), *W = malloc(blk * sizeof(double)), *V = malloc(blk * sizeof(double));
  int *perm = malloc((size_t)n * sizeof(int));
  if (!arena || !dense || !Z || !Y || !W || !V || !perm) FAIL("out of memory");
  if (cholamd_plan_fill_host(p, arena) || cholamd_plan_arena_to_dense(p, arena, dense)) FAIL("fill: %s", cholamd_last_error());
  cholamd_plan_perm(p, perm);
  for (size_t e = 0; e < blk; e++) { Z[e] = 1.0 + (double)((7919 * (int64_t)e) % 10) - 4.5; Y[e] = -7.0; }
  if (cholamd_plan_multiply_host_nrhs(p, arena, 2, Z, n, Y, n, K) != CHOLAMD_ERR_ARG || cholamd_plan_multiply_host_nrhs(p, arena, -2, Z, n, Y, n, K) != CHOLAMD_ERR_ARG ||
      cholamd_plan_multiply_host_nrhs(p, arena, 0, Z, n, Y, n, -1) != CHOLAMD_ERR_ARG || cholamd_plan_multiply_host_nrhs(p, arena, 0, Z, n - 1, Y, n, K) != CHOLAMD_ERR_ARG ||
      cholamd_plan_multiply_host_nrhs(p, arena, 1, Z, n, Y, n - 1, K) != CHOLAMD_ERR_ARG || cholamd_plan_multiply_host_nrhs(p, NULL, 0, Z, n, Y, n, K) != CHOLAMD_ERR_ARG ||
      cholamd_plan_multiply_host_nrhs(p, arena, 0, NULL, n, Y, n, K) != CHOLAMD_ERR_ARG || cholamd_plan_multiply_host_nrhs(p, arena, -1, Z, n, NULL, n, K) != CHOLAMD_ERR_ARG ||
      cholamd_plan_multiply_host_nrhs(NULL, arena, 0, Z, n, Y, n, K) != CHOLAMD_ERR_ARG)
    FAIL("multiply_host_nrhs accepts bad arguments");
  if (cholamd_plan_multiply_host_nrhs(p, NULL, 0, NULL, n, NULL, n, 0) != 0) FAIL("nrhs = 0 is not accepted");
  for (size_t e = 0; e < blk; e++) if (Y[e] != -7.0) FAIL("a refused multiply_host_nrhs wrote Y");
  for (int c = 0; c < 3; c++) {
    const int k = counts[c];
    for (int which = 0; which < 2; which++) {
      if (cholamd_plan_multiply_host_nrhs(p, arena, which, Z, n, Y, n, k)) FAIL("multiply_host_nrhs: %s", cholamd_last_error());
      for (int col = 0; col < k; col += (k > 2 ? k - 1 : 1)) { /* the first and the last column against the dense image */
        const double *z = Z + (size_t)col * n, *y = Y + (size_t)col * n;
        for (int i = 0; i < n; i++) {
          long double s = 0.0L, a = 0.0L;
          for (int j = 0; j < n; j++) {
            const double v = which == 0 ? (j <= i ? dense[i + (size_t)j * n] : 0.0) : (j >= i ? dense[j + (size_t)i * n] : 0.0);
            s += (long double)v * z[perm[j]];
            a += fabsl((long double)v * z[perm[j]]);
          }
          if (fabsl((long double)y[perm[i]] - s) > (n + 2) * 0x1p-53L * a) FAIL("which = %d, column %d of %d: y(%d) = %.17g, expected %.17Lg", which, col, k, perm[i], y[perm[i]], s);
        }
      }
      memcpy(W, Z, blk * sizeof(double));
      if (cholamd_plan_multiply_host_nrhs(p, arena, which, W, n, W, n, k)) FAIL("multiply_host_nrhs in place: %s", cholamd_last_error());
      if (memcmp(W, Y, (size_t)n * k * sizeof(double))) FAIL("which = %d, %d columns: the in-place product differs", which, k);
    }
    /* Y = the BACKWARD product (the last one computed); the full product is the FORWARD product of it */
    if (cholamd_plan_multiply_host_nrhs(p, arena, 0, Y, n, W, n, k) || cholamd_plan_multiply_host_nrhs(p, arena, -1, Z, n, V, n, k)) FAIL("full product: %s", cholamd_last_error());
    if (memcmp(W, V, (size_t)n * k * sizeof(double))) FAIL("%d columns: the full product is not FORWARD of BACKWARD", k);
  }
  free(perm); free(V); free(W); free(Y); free(Z); free(dense); free(arena);
  return 0;
}

int main(int argc, char **argv)
{
  if (argc < 4) { fprintf(stderr, "usage: multiply_nrhs_host matrix separators clusters [more triples]\n"); return 2; }
  for (int a = 1; a + 2 < argc; a += 3) {
    cholamd_plan *p = NULL;
    if (cholamd_plan_create(argv[a], argv[a + 1], argv[a + 2], &p)) { fprintf(stderr, "plan: %s\n", cholamd_last_error()); return 1; }
    if (run_plan(p)) return 1;
    cholamd_plan_destroy(p);
  }
  cholamd_problem *g = NULL;
  if (cholamd_generate_laplacian(12, 12, 12, 4, 16, &g)) { fprintf(stderr, "generate: %s\n", cholamd_last_error()); return 1; }
  cholamd_plan *p = NULL;
  if (cholamd_plan_create_from_problem(g, &p)) { fprintf(stderr, "problem plan: %s\n", cholamd_last_error()); return 1; }
  if (run_plan(p)) return 1;
  cholamd_plan_destroy(p);
  cholamd_problem_destroy(g);
  printf("multiply_nrhs_host: ok\n");
  return 0;
}
