/* The host restatement of the deterministic BLOCK solve (cholamd_plan_solve_det_host_nrhs) under the sanitizers, without an interpreter in the process:
 * `make asan` builds this against the sanitizer build and runs it with LeakSanitizer on.  The walk uses the block kernel's own index functions
 * (chol_muln_wave, chol_muln_elem of chol_plan.h), so an index of the kernel that leaves a strip leaves the host arena here -- which has EXACTLY the
 * plan's size -- and is the sanitizer's to report.  Plans of the fixtures and of a generated grid; B and X are nrhs columns at a leading dimension
 * ld = n + 3 > n in buffers of exactly ld * nrhs doubles.  As in solve_det_host.c the arena is the plain host fill, L = tril(P A P^T) stands in for a
 * factor, and
 *   which = 0:  L (P x) = P b,   which = 1:  L^T (P x) = P b,   which = -1:  L L^T (P x) = P b
 * is checked for every column by applying the dense image of the arena to x: the residual within (n + 2) u (|L| |y| + |b|) per row, the bound of a
 * substitution in any order (Higham, Thm 8.5) with the inner-product bound of the check itself.  Then, bit for bit: the halves compose to the whole
 * solve, in place gives the same bits, a column solved alone has the bits it has inside the block; the padding rows n .. ld - 1 of X are never written and
 * the refusals write nothing.  nrhs = 1 and 33: one column, and a full chunk followed by a chunk of one.  No GPU call is made. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "cholamd.h"

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)
#define PAD (-7.0)

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
static int pads_intact(const double *X, int n, int64_t ld, int k)
{
  for (int j = 0; j < k; j++)
    for (int64_t i = n; i < ld; i++) if (X[i + j * ld] != PAD) return 0;
  return 1;
}

static int run_plan(cholamd_plan *p, int K)
{
  const int n = cholamd_plan_n(p);
  const int64_t na = cholamd_plan_arena_doubles(p), ld = (int64_t)n + 3;
  const size_t blk = (size_t)ld * K;
  double *arena = malloc((size_t)na * sizeof(double)), *dense = malloc((size_t)n * n * sizeof(double));
  double *B = malloc(blk * sizeof(double)), *X = malloc(blk * sizeof(double)), *Y = malloc(blk * sizeof(double)), *W = malloc(blk * sizeof(double));
  double *b1 = malloc((size_t)n * sizeof(double)), *x1 = malloc((size_t)n * sizeof(double));
  long double *v = malloc((size_t)n * sizeof(long double)), *r = malloc((size_t)n * sizeof(long double)), *a = malloc((size_t)n * sizeof(long double)),
              *r2 = malloc((size_t)n * sizeof(long double)), *a2 = malloc((size_t)n * sizeof(long double));
  int *perm = malloc((size_t)n * sizeof(int));
  if (!arena || !dense || !B || !X || !Y || !W || !b1 || !x1 || !v || !r || !a || !r2 || !a2 || !perm) FAIL("out of memory");
  if (cholamd_plan_fill_host(p, arena) || cholamd_plan_arena_to_dense(p, arena, dense)) FAIL("fill: %s", cholamd_last_error());
  cholamd_plan_perm(p, perm);
  for (size_t e = 0; e < blk; e++) { B[e] = PAD; X[e] = PAD; }
  for (int j = 0; j < K; j++)
    for (int i = 0; i < n; i++) B[i + j * ld] = 1.0 + (double)((7919 * (int64_t)i + 104729 * (int64_t)j) % 10) - 4.5;
  if (cholamd_plan_solve_det_host_nrhs(p, arena, 2, B, ld, X, ld, K) != CHOLAMD_ERR_ARG || cholamd_plan_solve_det_host_nrhs(p, arena, -2, B, ld, X, ld, K) != CHOLAMD_ERR_ARG ||
      cholamd_plan_solve_det_host_nrhs(p, arena, 0, B, ld, X, ld, -1) != CHOLAMD_ERR_ARG || cholamd_plan_solve_det_host_nrhs(p, arena, 0, B, n - 1, X, ld, K) != CHOLAMD_ERR_ARG ||
      cholamd_plan_solve_det_host_nrhs(p, arena, 1, B, ld, X, n - 1, K) != CHOLAMD_ERR_ARG || cholamd_plan_solve_det_host_nrhs(p, NULL, 0, B, ld, X, ld, K) != CHOLAMD_ERR_ARG ||
      cholamd_plan_solve_det_host_nrhs(p, arena, 0, NULL, ld, X, ld, K) != CHOLAMD_ERR_ARG || cholamd_plan_solve_det_host_nrhs(p, arena, -1, B, ld, NULL, ld, K) != CHOLAMD_ERR_ARG ||
      cholamd_plan_solve_det_host_nrhs(NULL, arena, 0, B, ld, X, ld, K) != CHOLAMD_ERR_ARG)
    FAIL("solve_det_host_nrhs accepts bad arguments");
  if (cholamd_plan_solve_det_host_nrhs(p, NULL, 0, NULL, ld, NULL, ld, 0) != 0) FAIL("nrhs = 0 is not accepted");
  for (size_t e = 0; e < blk; e++) if (X[e] != PAD) FAIL("a refused solve_det_host_nrhs wrote X");
  for (int which = -1; which < 2; which++) {
    if (cholamd_plan_solve_det_host_nrhs(p, arena, which, B, ld, X, ld, K)) FAIL("solve_det_host_nrhs: %s", cholamd_last_error());
    if (!pads_intact(X, n, ld, K)) FAIL("which = %d: rows n .. ld - 1 of X were written", which);
    for (int j = 0; j < K; j++) {
      if (n > 1000 && j != 0 && j != 31 && j != K - 1) continue; /* (the dense check is n^2 per column: the ends of both chunks on the large fixture) */
      const double *b = B + j * ld, *x = X + j * ld;
      for (int i = 0; i < n; i++) v[i] = x[perm[i]];
      if (which == -1) { /* L (L^T v): the bound of the inner product carries through the outer one */
        apply(dense, n, 1, v, r2, a2);
        apply(dense, n, 0, r2, r, a);
        apply(dense, n, 0, a2, r2, a);
      } else apply(dense, n, which, v, r, a);
      for (int i = 0; i < n; i++) {
        const long double bound = (which == -1 ? 2 : 1) * (n + 2) * 0x1p-53L * (a[i] + fabsl((long double)b[perm[i]]));
        if (!(fabsl(r[i] - (long double)b[perm[i]]) <= bound)) FAIL("which = %d, column %d: residual of row %d is %.3Lg, bound %.3Lg", which, j, i, r[i] - (long double)b[perm[i]], bound);
      }
    }
    memcpy(W, B, blk * sizeof(double));
    if (cholamd_plan_solve_det_host_nrhs(p, arena, which, W, ld, W, ld, K)) FAIL("solve_det_host_nrhs in place: %s", cholamd_last_error());
    if (memcmp(W, X, blk * sizeof(double))) FAIL("which = %d: the in-place solve differs", which);
    /* the last column alone (a chunk of its own width, first position): the bits it has inside the block */
    memcpy(b1, B + (size_t)(K - 1) * ld, (size_t)n * sizeof(double));
    if (cholamd_plan_solve_det_host_nrhs(p, arena, which, b1, n, x1, n, 1)) FAIL("one column: %s", cholamd_last_error());
    if (memcmp(x1, X + (size_t)(K - 1) * ld, (size_t)n * sizeof(double))) FAIL("which = %d: column %d alone differs from the column inside the block", which, K - 1);
    if (which == -1) memcpy(Y, X, blk * sizeof(double));
  }
  if (cholamd_plan_solve_det_host_nrhs(p, arena, 0, B, ld, W, ld, K) || cholamd_plan_solve_det_host_nrhs(p, arena, 1, W, ld, W, ld, K)) FAIL("halves: %s", cholamd_last_error());
  if (memcmp(W, Y, blk * sizeof(double))) FAIL("BACKWARD of FORWARD differs from the whole solve");
  free(perm); free(a2); free(r2); free(a); free(r); free(v); free(x1); free(b1); free(W); free(Y); free(X); free(B); free(dense); free(arena);
  return 0;
}

int main(int argc, char **argv)
{
  static const int counts[2] = { 1, 33 };
  if (argc < 4) { fprintf(stderr, "usage: solve_det_nrhs_host matrix separators clusters [more triples]\n"); return 2; }
  for (int a = 1; a + 2 < argc; a += 3) {
    cholamd_plan *p = NULL;
    if (cholamd_plan_create(argv[a], argv[a + 1], argv[a + 2], &p)) { fprintf(stderr, "plan: %s\n", cholamd_last_error()); return 1; }
    for (int c = 0; c < 2; c++) if (run_plan(p, counts[c])) return 1;
    cholamd_plan_destroy(p);
  }
  cholamd_problem *g = NULL;
  if (cholamd_generate_laplacian(12, 12, 12, 4, 16, &g)) { fprintf(stderr, "generate: %s\n", cholamd_last_error()); return 1; }
  cholamd_plan *p = NULL;
  if (cholamd_plan_create_from_problem(g, &p)) { fprintf(stderr, "problem plan: %s\n", cholamd_last_error()); return 1; }
  for (int c = 0; c < 2; c++) if (run_plan(p, counts[c])) return 1;
  cholamd_plan_destroy(p);
  cholamd_problem_destroy(g);
  printf("solve_det_nrhs_host: ok\n");
  return 0;
}
