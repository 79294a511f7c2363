/* The host restatement of the deterministic streamed solve (cholamd_plan_solve_det_host) and its list views under the sanitizers, without an
 * interpreter in the process: `make asan` builds this against the sanitizer build and runs it with LeakSanitizer on.  Plans of the fixtures and of a
 * generated grid, exact-size buffers (an access past them is the sanitizer's to report).  The arena is the plain host fill: L = tril(P A P^T) stands in
 * for a factor (it lies inside the envelope the leaf skips assume, and a Laplacian's diagonal dominance keeps the substitutions tame), so
 *   which = 0:  x solves L (P x) = P b,   which = 1:  L^T (P x) = P b,   which = -1:  L L^T (P x) = P b
 * and each is checked by applying the dense image of the arena to x: the residual against b within (n + 2) u (|L| |y| + |b|) per row -- the bound of
 * a substitution in any order (Higham, Thm 8.5) with the inner-product bound of the check itself.  Then: the halves compose to the whole solve bit for
 * bit, in place gives the same bits, the counts match the lists, the refusals write nothing.  No GPU call is made. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "cholamd.h"

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

/* r = T v with T = tril(dense) (trans = 0) or its transpose (1), permuted coordinates; a = |T| |v| */
static void apply(const double *dense, int n, int trans, const long double *v, long double *r, long double *a)
{
  for (int i = 0; i < n; i++) {
    long double s = 0.0L, t = 0.0L;
    for (int j = 0; j < n; j++) {
      const double e = !trans ? (j <= i ? dense[i + (size_t)j * n] : 0.0) : (j >= i ? dense[j + (size_t)i * n] : 0.0);
      s += (long double)e * v[j];
      t += fabsl((long double)e * v[j]);
    }
    r[i] = s; a[i] = t;
  }
}

static int run_plan(cholamd_plan *p)
{
  const int n = cholamd_plan_n(p);
  const int64_t na = cholamd_plan_arena_doubles(p);
  double *arena = malloc((size_t)na * sizeof(double)), *dense = malloc((size_t)n * n * sizeof(double));
  double *b = malloc((size_t)n * sizeof(double)), *x = malloc((size_t)n * sizeof(double)), *y = malloc((size_t)n * sizeof(double)), *w = malloc((size_t)n * sizeof(double));
  long double *v = malloc((size_t)n * sizeof(long double)), *r = malloc((size_t)n * sizeof(long double)), *a = malloc((size_t)n * sizeof(long double)),
              *r2 = malloc((size_t)n * sizeof(long double)), *a2 = malloc((size_t)n * sizeof(long double));
  int *perm = malloc((size_t)n * sizeof(int));
  if (!arena || !dense || !b || !x || !y || !w || !v || !r || !a || !r2 || !a2 || !perm) FAIL("out of memory");
  if (cholamd_plan_fill_host(p, arena) || cholamd_plan_arena_to_dense(p, arena, dense)) FAIL("fill: %s", cholamd_last_error());
  cholamd_plan_perm(p, perm);
  for (int i = 0; i < n; i++) { b[i] = 1.0 + (double)((7919 * (int64_t)i) % 10) - 4.5; x[i] = -7.0; }
  if (cholamd_plan_solve_det_host(p, arena, 2, b, x) != CHOLAMD_ERR_ARG || cholamd_plan_solve_det_host(p, arena, -2, b, x) != CHOLAMD_ERR_ARG ||
      cholamd_plan_solve_det_host(p, NULL, 0, b, x) != CHOLAMD_ERR_ARG || cholamd_plan_solve_det_host(p, arena, 0, NULL, x) != CHOLAMD_ERR_ARG ||
      cholamd_plan_solve_det_host(p, arena, 1, b, NULL) != CHOLAMD_ERR_ARG || cholamd_plan_solve_det_host(NULL, arena, 0, b, x) != CHOLAMD_ERR_ARG)
    FAIL("solve_det_host accepts bad arguments");
  for (int i = 0; i < n; i++) if (x[i] != -7.0) FAIL("a refused solve_det_host wrote x");
  for (int which = -1; which < 2; which++) {
    if (cholamd_plan_solve_det_host(p, arena, which, b, x)) FAIL("solve_det_host: %s", cholamd_last_error());
    for (int i = 0; i < n; i++) v[i] = x[perm[i]];
    if (which == -1) { /* L (L^T v): the bound of the inner product carries through the outer one */
      apply(dense, n, 1, v, r2, a2);
      apply(dense, n, 0, r2, r, a);
      apply(dense, n, 0, a2, r2, a);
    } else apply(dense, n, which, v, r, a);
    for (int i = 0; i < n; i++) {
      const long double bound = (which == -1 ? 2 : 1) * (n + 2) * 0x1p-53L * (a[i] + fabsl((long double)b[perm[i]]));
      if (!(fabsl(r[i] - (long double)b[perm[i]]) <= bound)) FAIL("which = %d: residual of row %d is %.3Lg, bound %.3Lg", which, i, r[i] - (long double)b[perm[i]], bound);
    }
    memcpy(w, b, (size_t)n * sizeof(double));
    if (cholamd_plan_solve_det_host(p, arena, which, w, w)) FAIL("solve_det_host in place: %s", cholamd_last_error());
    if (memcmp(w, x, (size_t)n * sizeof(double))) FAIL("which = %d: the in-place solve differs", which);
    if (which == -1) memcpy(y, x, (size_t)n * sizeof(double));
  }
  if (cholamd_plan_solve_det_host(p, arena, 0, b, w) || cholamd_plan_solve_det_host(p, arena, 1, w, w)) FAIL("halves: %s", cholamd_last_error());
  if (memcmp(w, y, (size_t)n * sizeof(double))) FAIL("BACKWARD of FORWARD differs from the whole solve");
  int64_t cnt[8];
  if (cholamd_plan_solve_det_counts(p, cnt)) FAIL("counts: %s", cholamd_last_error());
  if (cholamd_plan_solve_det_counts(p, NULL) != CHOLAMD_ERR_ARG || cholamd_plan_solve_det_counts(NULL, cnt) != CHOLAMD_ERR_ARG) FAIL("counts accepts bad arguments");
  for (int which = 0; which < 2; which++) { /* exact-size list buffers; every position solved once by the spans is the builder's own check */
    const int64_t ns = cnt[4 * which], ni = cnt[4 * which + 1], nq = cnt[4 * which + 2];
    int64_t *steps = malloc((size_t)(ns > 0 ? ns : 1) * 4 * sizeof(int64_t)), *items = malloc((size_t)(ni > 0 ? ni : 1) * 4 * sizeof(int64_t)),
            *srcs = malloc((size_t)(nq > 0 ? nq : 1) * 5 * sizeof(int64_t));
    if (!steps || !items || !srcs) FAIL("out of memory");
    if (cholamd_plan_solve_det_lists(p, which, steps, items, srcs)) FAIL("lists: %s", cholamd_last_error());
    if (cholamd_plan_solve_det_lists(p, 2, steps, items, srcs) != CHOLAMD_ERR_ARG || cholamd_plan_solve_det_lists(p, which, NULL, items, srcs) != CHOLAMD_ERR_ARG) FAIL("lists accepts bad arguments");
    int64_t at = 0, sat = 0;
    for (int64_t t = 0; t < ns; t++) {
      if (steps[4 * t + 2] != at || steps[4 * t + 3] < at || (steps[4 * t + 1] != -1 && steps[4 * t + 1] % 256)) FAIL("which = %d: step %lld is out of order", which, (long long)t);
      at = steps[4 * t + 3];
    }
    if (at != ni) FAIL("which = %d: the steps cover %lld of %lld items", which, (long long)at, (long long)ni);
    for (int64_t i = 0; i < ni; i++) {
      if (items[4 * i + 2] != sat || items[4 * i + 3] <= sat || items[4 * i + 1] < 1 || items[4 * i + 1] > 16) FAIL("which = %d: item %lld is malformed", which, (long long)i);
      sat = items[4 * i + 3];
    }
    if (sat != nq) FAIL("which = %d: the items cover %lld of %lld sources", which, (long long)sat, (long long)nq);
    free(steps); free(items); free(srcs);
  }
  free(perm); free(a2); free(r2); free(a); free(r); free(v); free(w); free(y); free(x); free(b); free(dense); free(arena);
  return 0;
}

int main(int argc, char **argv)
{
  if (argc < 4) { fprintf(stderr, "usage: solve_det_host matrix separators clusters [more triples]\n"); return 2; }
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
  printf("solve_det_host: ok\n");
  return 0;
}
