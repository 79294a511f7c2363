/* The host restatement of the forward products with the factor (cholamd_plan_multiply_host) under the sanitizers, without an interpreter in the
 * process: `make asan` builds this against the sanitizer build and runs it with LeakSanitizer on.  Plans of the fixtures and of a generated grid,
 * exact-size buffers (an access past them is the sanitizer's to report), both directions, in place, the refusals.  The arena is the plain host fill:
 * tril(P A P^T) stands in for L (it lies inside the envelope the leaf skips assume), so the product is checked against the dense image of the arena
 * with the inner-product bound (k + 2) u |L| |z|, k <= n.  No GPU call is made. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "cholamd.h"

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

static int run_plan(cholamd_plan *p)
{
  const int n = cholamd_plan_n(p);
  const int64_t na = cholamd_plan_arena_doubles(p);
  double *arena = malloc((size_t)na * sizeof(double)), *dense = malloc((size_t)n * n * sizeof(double));
  double *z = malloc((size_t)n * sizeof(double)), *y = malloc((size_t)n * sizeof(double)), *w = malloc((size_t)n * sizeof(double));
  int *perm = malloc((size_t)n * sizeof(int));
  if (!arena || !dense || !z || !y || !w || !perm) FAIL("out of memory");
  if (cholamd_plan_fill_host(p, arena) || cholamd_plan_arena_to_dense(p, arena, dense)) FAIL("fill: %s", cholamd_last_error());
  cholamd_plan_perm(p, perm);
  for (int i = 0; i < n; i++) { z[i] = 1.0 + (double)((7919 * (int64_t)i) % 10) - 4.5; y[i] = -7.0; }
  if (cholamd_plan_multiply_host(p, arena, 2, z, y) != CHOLAMD_ERR_ARG || cholamd_plan_multiply_host(p, arena, -1, z, y) != CHOLAMD_ERR_ARG ||
      cholamd_plan_multiply_host(p, NULL, 0, z, y) != CHOLAMD_ERR_ARG || cholamd_plan_multiply_host(p, arena, 0, NULL, y) != CHOLAMD_ERR_ARG ||
      cholamd_plan_multiply_host(p, arena, 1, z, NULL) != CHOLAMD_ERR_ARG || cholamd_plan_multiply_host(NULL, arena, 0, z, y) != CHOLAMD_ERR_ARG)
    FAIL("multiply_host accepts bad arguments");
  for (int i = 0; i < n; i++) if (y[i] != -7.0) FAIL("a refused multiply_host wrote y");
  for (int which = 0; which < 2; which++) {
    if (cholamd_plan_multiply_host(p, arena, which, z, y)) FAIL("multiply_host: %s", cholamd_last_error());
    for (int i = 0; i < n; i++) { /* row i of tril(dense) (FORWARD) or of its transpose (BACKWARD), permuted coordinates */
      long double s = 0.0L, a = 0.0L;
      for (int j = 0; j < n; j++) {
        const double v = which == 0 ? (j <= i ? dense[i + (size_t)j * n] : 0.0) : (j >= i ? dense[j + (size_t)i * n] : 0.0);
        s += (long double)v * z[perm[j]];
        a += fabsl((long double)v * z[perm[j]]);
      }
      if (fabsl((long double)y[perm[i]] - s) > (n + 2) * 0x1p-53L * a) FAIL("which = %d: y(%d) = %.17g, expected %.17Lg", which, perm[i], y[perm[i]], s);
    }
    memcpy(w, z, (size_t)n * sizeof(double));
    if (cholamd_plan_multiply_host(p, arena, which, w, w)) FAIL("multiply_host in place: %s", cholamd_last_error());
    if (memcmp(w, y, (size_t)n * sizeof(double))) FAIL("which = %d: the in-place product differs", which);
  }
  free(perm); free(w); free(y); free(z); free(dense); free(arena);
  return 0;
}

int main(int argc, char **argv)
{
  if (argc < 4) { fprintf(stderr, "usage: multiply_host matrix separators clusters [more triples]\n"); return 2; }
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
  printf("multiply_host: ok\n");
  return 0;
}
