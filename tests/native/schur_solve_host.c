/* The host restatement of the block Schur condense / expand (cholamd_plan_schur_condense_host_nrhs / _expand_host_nrhs, cholamd_plan_schur_det_counts /
 * _lists) under the sanitizers, without an interpreter in the process: `make schur_solve_host` builds this against the sanitizer build and runs it with
 * LeakSanitizer on.  A generated 12^3 grid, every k the tree allows, exact-size buffers (an access past them is the sanitizer's to report), the refusals.
 * The arena is the plain fill: its stored lower triangle T = tril(P A P^T) has a positive diagonal, and the sweeps are triangular solves with whatever
 * the arena holds, so the results are checked against T itself: T_II w_I = b_I, g = b_T - T_TI w_I, and T_II^T x_I = w_I - T_TI^T x_T.  No GPU call. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "cholamd.h"

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)
#define NRHS 33

static int run_plan(cholamd_plan *p)
{
  const int L = cholamd_plan_levels(p), n = cholamd_plan_n(p);
  const int64_t na = cholamd_plan_arena_doubles(p);
  double *arena = malloc((size_t)na * sizeof(double)), *T = malloc((size_t)n * n * sizeof(double));
  int *perm = malloc((size_t)n * sizeof(int));
  if (!arena || !T || !perm) FAIL("out of memory");
  if (cholamd_plan_fill_host(p, arena) || cholamd_plan_arena_to_dense(p, arena, T)) FAIL("fill: %s", cholamd_last_error());
  cholamd_plan_perm(p, perm);
  double *B = malloc((size_t)n * NRHS * sizeof(double)), *W = malloc((size_t)n * NRHS * sizeof(double)), *X = malloc((size_t)n * NRHS * sizeof(double));
  if (!B || !W || !X) FAIL("out of memory");
  for (int64_t i = 0; i < (int64_t)n * NRHS; i++) B[i] = sin(0.37 * (double)i) + 0.01 * (double)(i % 7);
  int64_t cnt[8];
  if (cholamd_plan_schur_det_counts(p, 0, cnt) != CHOLAMD_ERR_ARG || cholamd_plan_schur_det_counts(p, L, cnt) != CHOLAMD_ERR_ARG ||
      cholamd_plan_schur_det_counts(p, 1, NULL) != CHOLAMD_ERR_ARG || cholamd_plan_schur_det_counts(NULL, 1, cnt) != CHOLAMD_ERR_ARG)
    FAIL("schur_det_counts accepts bad arguments");
  for (int k = 1; k <= L - 1; k++) {
    const int m = cholamd_plan_schur_size(p, k), t0 = n - m;
    if (m <= 0 || m >= n) FAIL("schur_size(%d) = %d", k, m);
    if (cholamd_plan_schur_det_counts(p, k, cnt)) FAIL("counts: %s", cholamd_last_error());
    for (int q = 0; q < 2; q++) { /* the lists into exact-size buffers; every source stays inside the arena and the vector */
      int64_t *steps = malloc((size_t)(cnt[4 * q] + 1) * 4 * sizeof(int64_t)), *items = malloc((size_t)(cnt[4 * q + 1] + 1) * 4 * sizeof(int64_t)),
              *srcs = malloc((size_t)(cnt[4 * q + 2] + 1) * 5 * sizeof(int64_t));
      if (!steps || !items || !srcs) FAIL("out of memory");
      if (cholamd_plan_schur_det_lists(p, k, 2, steps, items, srcs) != CHOLAMD_ERR_ARG || cholamd_plan_schur_det_lists(p, k, q, NULL, items, srcs) != CHOLAMD_ERR_ARG)
        FAIL("schur_det_lists accepts bad arguments");
      if (cholamd_plan_schur_det_lists(p, k, q, steps, items, srcs)) FAIL("lists: %s", cholamd_last_error());
      int lead = 0;
      for (int64_t t = 0; t < cnt[4 * q]; t++) {
        lead += steps[4 * t] == -1;
        if (steps[4 * t] != -1 && steps[4 * t] < k) FAIL("step %lld of k = %d lies above the cut", (long long)t, k);
        for (int64_t i = steps[4 * t + 2]; i < steps[4 * t + 3]; i++)
          for (int64_t e = items[4 * i + 2]; e < items[4 * i + 3]; e++) {
            const int64_t *s = srcs + 5 * e, nv = items[4 * i + 1];
            const int64_t last = q == 0 ? s[0] + nv - 1 + (s[2] - 1) * s[1] : s[0] + s[2] - 1 + (nv - 1) * s[1];
            if (s[0] < 0 || last >= na || s[3] < 0 || s[3] + s[2] > n) FAIL("source %lld of k = %d leaves the arena or the vector", (long long)e, k);
            if (steps[4 * t] == -1 && s[3] + s[2] > t0) FAIL("kept-lead source %lld of k = %d reads above the cut", (long long)e, k);
          }
      }
      if (lead != (q == 0)) FAIL("%d kept lead steps in direction %d", lead, q);
      free(steps); free(items); free(srcs);
    }
    double *G = malloc((size_t)m * NRHS * sizeof(double)), *XT = malloc((size_t)m * NRHS * sizeof(double));
    if (!G || !XT) FAIL("out of memory");
    for (int64_t i = 0; i < (int64_t)n * NRHS; i++) W[i] = X[i] = -7.0;
    for (int64_t i = 0; i < (int64_t)m * NRHS; i++) { G[i] = -7.0; XT[i] = cos(0.11 * (double)i); }
    /* the refusals write nothing */
    if (cholamd_plan_schur_condense_host_nrhs(p, k, arena, B, n - 1, W, n, G, m, NRHS) != CHOLAMD_ERR_ARG ||
        cholamd_plan_schur_condense_host_nrhs(p, k, arena, B, n, W, n, G, m - 1, NRHS) != CHOLAMD_ERR_ARG ||
        cholamd_plan_schur_condense_host_nrhs(p, k, arena, B, n, NULL, n, G, m, NRHS) != CHOLAMD_ERR_ARG ||
        cholamd_plan_schur_condense_host_nrhs(p, k, NULL, B, n, W, n, G, m, NRHS) != CHOLAMD_ERR_ARG ||
        cholamd_plan_schur_condense_host_nrhs(p, k, arena, B, n, W, n, G, m, -1) != CHOLAMD_ERR_ARG ||
        cholamd_plan_schur_condense_host_nrhs(p, L, arena, B, n, W, n, G, m, NRHS) != CHOLAMD_ERR_ARG ||
        cholamd_plan_schur_expand_host_nrhs(p, k, arena, W, n, XT, m - 1, X, n, NRHS) != CHOLAMD_ERR_ARG ||
        cholamd_plan_schur_expand_host_nrhs(p, k, arena, W, n, XT, m, X, n - 1, NRHS) != CHOLAMD_ERR_ARG ||
        cholamd_plan_schur_expand_host_nrhs(p, k, arena, W, n, NULL, m, X, n, NRHS) != CHOLAMD_ERR_ARG ||
        cholamd_plan_schur_expand_host_nrhs(p, 0, arena, W, n, XT, m, X, n, NRHS) != CHOLAMD_ERR_ARG)
      FAIL("a bad argument is accepted (k = %d)", k);
    if (cholamd_plan_schur_condense_host_nrhs(p, k, NULL, NULL, n, NULL, n, NULL, m, 0) || cholamd_plan_schur_expand_host_nrhs(p, k, NULL, NULL, n, NULL, m, NULL, n, 0))
      FAIL("nrhs = 0 is refused");
    for (int64_t i = 0; i < (int64_t)n * NRHS; i++) if (W[i] != -7.0 || X[i] != -7.0) FAIL("a refused call wrote W or X");
    for (int64_t i = 0; i < (int64_t)m * NRHS; i++) if (G[i] != -7.0) FAIL("a refused call wrote G");
    if (cholamd_plan_schur_condense_host_nrhs(p, k, arena, B, n, W, n, G, m, NRHS)) FAIL("condense: %s", cholamd_last_error());
    if (cholamd_plan_schur_expand_host_nrhs(p, k, arena, W, n, XT, m, X, n, NRHS)) FAIL("expand: %s", cholamd_last_error());
    for (int j = 0; j < NRHS; j += 16) { /* columns 0, 16, 32: both halves of a tile and the second chunk */
      const double *b = B + (size_t)j * n, *w = W + (size_t)j * n, *g = G + (size_t)j * m, *xt = XT + (size_t)j * m, *x = X + (size_t)j * n;
      double worst = 0.0, scale = 0.0;
      for (int i = 0; i < n; i++) { /* rows of the forward sweep: T(i, 0 .. min(i, t0 - 1)) w = b_i (- g_i above the cut) */
        double acc = 0.0, mag = 0.0;
        for (int c = 0; c < t0 && c <= i; c++) { acc += T[i + (size_t)c * n] * w[c]; mag += fabs(T[i + (size_t)c * n] * w[c]); }
        const double want = i < t0 ? b[perm[i]] : b[perm[i]] - g[i - t0];
        if (i >= t0 && w[i] != g[i - t0]) FAIL("the tail of W is not G (k = %d)", k);
        if (fabs(acc - want) > worst) worst = fabs(acc - want);
        if (mag + fabs(want) > scale) scale = mag + fabs(want);
      }
      for (int c = 0; c < t0; c++) { /* columns of the backward sweep: sum_{i >= c} T(i, c) y_i = w_c with y = the permuted x */
        double acc = 0.0, mag = 0.0;
        for (int i = c; i < n; i++) { acc += T[i + (size_t)c * n] * x[perm[i]]; mag += fabs(T[i + (size_t)c * n] * x[perm[i]]); }
        if (fabs(acc - w[c]) > worst) worst = fabs(acc - w[c]);
        if (mag + fabs(w[c]) > scale) scale = mag + fabs(w[c]);
      }
      for (int i = t0; i < n; i++) if (x[perm[i]] != xt[i - t0]) FAIL("the kept part of X is not XT (k = %d)", k);
      if (!(worst <= 1e-11 * scale)) FAIL("k = %d column %d: the sweeps miss their triangular systems by %g (scale %g)", k, j, worst, scale);
    }
    /* a column alone has the bits it has in the block */
    double *w1 = malloc((size_t)n * sizeof(double)), *g1 = malloc((size_t)m * sizeof(double)), *x1 = malloc((size_t)n * sizeof(double));
    if (!w1 || !g1 || !x1) FAIL("out of memory");
    if (cholamd_plan_schur_condense_host_nrhs(p, k, arena, B + (size_t)32 * n, n, w1, n, g1, m, 1) ||
        cholamd_plan_schur_expand_host_nrhs(p, k, arena, W + (size_t)17 * n, n, XT + (size_t)17 * m, m, x1, n, 1))
      FAIL("single column: %s", cholamd_last_error());
    if (memcmp(w1, W + (size_t)32 * n, (size_t)n * sizeof(double)) || memcmp(g1, G + (size_t)32 * m, (size_t)m * sizeof(double)) ||
        memcmp(x1, X + (size_t)17 * n, (size_t)n * sizeof(double)))
      FAIL("a column alone differs from the column in the block (k = %d)", k);
    free(w1); free(g1); free(x1); free(G); free(XT);
  }
  free(B); free(W); free(X); free(perm); free(T); free(arena);
  return 0;
}

int main(void)
{
  cholamd_problem *g = NULL;
  if (cholamd_generate_laplacian(12, 12, 12, 4, 16, &g)) { fprintf(stderr, "generate: %s\n", cholamd_last_error()); return 1; }
  cholamd_plan *p = NULL;
  if (cholamd_plan_create_from_problem(g, &p)) { fprintf(stderr, "problem plan: %s\n", cholamd_last_error()); return 1; }
  if (run_plan(p)) return 1;
  cholamd_plan_destroy(p);
  cholamd_problem_destroy(g);
  if (cholamd_plan_schur_condense_host_nrhs(NULL, 1, NULL, NULL, 1, NULL, 1, NULL, 1, 1) != CHOLAMD_ERR_ARG) return 1;
  printf("schur_solve_host: ok\n");
  return 0;
}
