/* The pruned step lists of the sparse solve and their host walk (cholamd_plan_sparse_counts / _lists / _solve_host_nrhs) under the sanitizers, without an
 * interpreter in the process: `make sparse_solve_host` builds this against the sanitizer build and runs it with LeakSanitizer on.  A generated 12^3 grid
 * of 4 levels; the dof sets A (one dof of the first leaf), E (in: the first leaf, out: the last leaf -- the paths meet at the root only) and H (everything);
 * exact-size buffers (an access past them is the sanitizer's to report); the refusals.  The arena is the plain fill: its stored lower triangle
 * T = tril(P A P^T) has a positive diagonal and the sweeps are triangular solves with whatever the arena holds, so the results are compared with this
 * file's own dense substitution T y = P b, T^T z = y on the scattered right-hand side.  No GPU call. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "cholamd.h"

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)
#define NRHS 33

static int run_set(cholamd_plan *p, const double *arena, const double *T, const int *perm, char set, const int *in, int n_in, const int *out, int n_out, const int64_t full[8])
{
  const int n = cholamd_plan_n(p), L = cholamd_plan_levels(p), ns = cholamd_plan_num_separators(p);
  const int64_t na = cholamd_plan_arena_doubles(p);
  int64_t cnt[12];
  if (cholamd_plan_sparse_counts(p, in, n_in, out, n_out, cnt)) FAIL("set %c counts: %s", set, cholamd_last_error());
  for (int q = 0; q < 2; q++) {
    const int64_t want_seps = set == 'H' ? ns : L;
    if (cnt[5 * q] != want_seps) FAIL("set %c direction %d: %lld active separators, not %lld", set, q, (long long)cnt[5 * q], (long long)want_seps);
    if (set == 'H' ? (cnt[5 * q + 1] != full[4 * q] || cnt[5 * q + 2] != full[4 * q + 1] || cnt[5 * q + 3] != full[4 * q + 2] || cnt[5 * q + 4] != full[4 * q + 3])
                   : cnt[5 * q + 4] >= full[4 * q + 3])
      FAIL("set %c direction %d: the counts are not %s the full lists'", set, q, set == 'H' ? "equal to" : "below");
    /* the lists into exact-size buffers; every source stays inside the arena and the vector */
    int64_t *steps = malloc((size_t)(cnt[5 * q + 1] + 1) * 4 * sizeof(int64_t)), *items = malloc((size_t)(cnt[5 * q + 2] + 1) * 4 * sizeof(int64_t)),
            *srcs = malloc((size_t)(cnt[5 * q + 3] + 1) * 5 * sizeof(int64_t));
    if (!steps || !items || !srcs) FAIL("out of memory");
    if (cholamd_plan_sparse_lists(p, in, n_in, out, n_out, 2, steps, items, srcs) != CHOLAMD_ERR_ARG || cholamd_plan_sparse_lists(p, in, n_in, out, n_out, q, NULL, items, srcs) != CHOLAMD_ERR_ARG)
      FAIL("sparse_lists accepts bad arguments");
    if (cholamd_plan_sparse_lists(p, in, n_in, out, n_out, q, steps, items, srcs)) FAIL("set %c lists: %s", set, cholamd_last_error());
    for (int64_t t = 0; t < cnt[5 * q + 1]; t++)
      for (int64_t i = steps[4 * t + 2]; i < steps[4 * t + 3]; i++)
        for (int64_t e = items[4 * i + 2]; e < items[4 * i + 3]; e++) {
          const int64_t *s = srcs + 5 * e, nv = items[4 * i + 1];
          const int64_t last = q == 0 ? s[0] + nv - 1 + (s[2] - 1) * s[1] : s[0] + s[2] - 1 + (nv - 1) * s[1];
          if (s[0] < 0 || last >= na || s[3] < 0 || s[3] + s[2] > n) FAIL("set %c: source %lld leaves the arena or the vector", set, (long long)e);
        }
    free(steps); free(items); free(srcs);
  }
  if (cnt[10] < 1 || cnt[10] > n || (set == 'H' && (cnt[10] != n || cnt[11] != 1))) FAIL("set %c: %lld active positions in %lld ranges", set, (long long)cnt[10], (long long)cnt[11]);
  double *Bs = malloc((size_t)n_in * NRHS * sizeof(double)), *Xs = malloc((size_t)n_out * NRHS * sizeof(double)), *y = malloc((size_t)n * sizeof(double));
  if (!Bs || !Xs || !y) FAIL("out of memory");
  for (int64_t i = 0; i < (int64_t)n_in * NRHS; i++) Bs[i] = sin(0.37 * (double)i) + 0.01 * (double)(i % 7) + 0.5;
  for (int64_t i = 0; i < (int64_t)n_out * NRHS; i++) Xs[i] = -7.0;
  /* the refusals write nothing */
  if (cholamd_plan_sparse_solve_host_nrhs(p, arena, in, n_in, out, n_out, -1, Bs, n_in - 1, Xs, n_out, NRHS) != CHOLAMD_ERR_ARG ||
      cholamd_plan_sparse_solve_host_nrhs(p, arena, in, n_in, out, n_out, -1, Bs, n_in, Xs, n_out - 1, NRHS) != CHOLAMD_ERR_ARG ||
      cholamd_plan_sparse_solve_host_nrhs(p, arena, in, n_in, out, n_out, 2, Bs, n_in, Xs, n_out, NRHS) != CHOLAMD_ERR_ARG ||
      cholamd_plan_sparse_solve_host_nrhs(p, NULL, in, n_in, out, n_out, -1, Bs, n_in, Xs, n_out, NRHS) != CHOLAMD_ERR_ARG ||
      cholamd_plan_sparse_solve_host_nrhs(p, arena, in, n_in, out, n_out, -1, Bs, n_in, NULL, n_out, NRHS) != CHOLAMD_ERR_ARG ||
      cholamd_plan_sparse_solve_host_nrhs(p, arena, in, n_in, out, n_out, -1, Bs, n_in, Xs, n_out, -1) != CHOLAMD_ERR_ARG ||
      cholamd_plan_sparse_solve_host_nrhs(p, arena, in, 0, out, n_out, -1, Bs, n_in, Xs, n_out, NRHS) != CHOLAMD_ERR_ARG ||
      cholamd_plan_sparse_solve_host_nrhs(p, arena, NULL, n_in, out, n_out, -1, Bs, n_in, Xs, n_out, NRHS) != CHOLAMD_ERR_ARG)
    FAIL("set %c: a bad argument is accepted", set);
  if (cholamd_plan_sparse_solve_host_nrhs(p, NULL, in, n_in, out, n_out, -1, NULL, n_in, NULL, n_out, 0)) FAIL("nrhs = 0 is refused");
  for (int64_t i = 0; i < (int64_t)n_out * NRHS; i++) if (Xs[i] != -7.0) FAIL("set %c: a refused call wrote Xs", set);
  if (cholamd_plan_sparse_solve_host_nrhs(p, arena, in, n_in, out, n_out, -1, Bs, n_in, Xs, n_out, NRHS)) FAIL("set %c solve: %s", set, cholamd_last_error());
  int *iperm = malloc((size_t)n * sizeof(int));
  if (!iperm) FAIL("out of memory");
  for (int i = 0; i < n; i++) iperm[perm[i]] = i;
  for (int j = 0; j < NRHS; j += 16) { /* columns 0, 16, 32: both halves of a tile and the second chunk */
    memset(y, 0, (size_t)n * sizeof(double));
    for (int i = 0; i < n_in; i++) y[iperm[in[i]]] = Bs[i + (size_t)j * n_in];
    for (int i = 0; i < n; i++) { /* T y = P b, then T^T z = y, in place */
      double v = y[i];
      for (int c = 0; c < i; c++) v -= T[i + (size_t)c * n] * y[c];
      y[i] = v / T[i + (size_t)i * n];
    }
    for (int i = n - 1; i >= 0; i--) {
      double v = y[i];
      for (int r = i + 1; r < n; r++) v -= T[r + (size_t)i * n] * y[r];
      y[i] = v / T[i + (size_t)i * n];
    }
    double worst = 0.0, scale = 0.0;
    for (int i = 0; i < n; i++) if (fabs(y[i]) > scale) scale = fabs(y[i]);
    for (int i = 0; i < n_out; i++) {
      const double d = fabs(Xs[i + (size_t)j * n_out] - y[iperm[out[i]]]);
      if (!(d <= worst)) worst = d;
    }
    if (!(worst <= 1e-11 * scale)) FAIL("set %c column %d: the walk misses the dense substitution by %g (scale %g)", set, j, worst, scale);
  }
  /* a column alone has the bits it has in the block */
  double *x1 = malloc((size_t)n_out * sizeof(double));
  if (!x1) FAIL("out of memory");
  if (cholamd_plan_sparse_solve_host_nrhs(p, arena, in, n_in, out, n_out, -1, Bs + (size_t)32 * n_in, n_in, x1, n_out, 1)) FAIL("single column: %s", cholamd_last_error());
  if (memcmp(x1, Xs + (size_t)32 * n_out, (size_t)n_out * sizeof(double))) FAIL("set %c: a column alone differs from the column in the block", set);
  free(x1); free(iperm); free(Bs); free(Xs); free(y);
  return 0;
}

static int run_plan(cholamd_plan *p)
{
  const int n = cholamd_plan_n(p), L = cholamd_plan_levels(p), ns = cholamd_plan_num_separators(p);
  const int64_t na = cholamd_plan_arena_doubles(p);
  double *arena = malloc((size_t)na * sizeof(double)), *T = malloc((size_t)n * n * sizeof(double));
  int *perm = malloc((size_t)n * sizeof(int)), *tree = malloc((size_t)ns * sizeof(int)), *off = malloc((size_t)ns * sizeof(int)), *size = malloc((size_t)ns * sizeof(int)),
      *all = malloc((size_t)n * sizeof(int));
  if (!arena || !T || !perm || !tree || !off || !size || !all) FAIL("out of memory");
  if (cholamd_plan_fill_host(p, arena) || cholamd_plan_arena_to_dense(p, arena, T)) FAIL("fill: %s", cholamd_last_error());
  cholamd_plan_perm(p, perm); cholamd_plan_tree(p, tree); cholamd_plan_sep_offsets(p, off); cholamd_plan_sep_sizes(p, size);
  for (int i = 0; i < n; i++) all[i] = i;
  int64_t full[8];
  if (cholamd_plan_solve_det_counts(p, full)) FAIL("solve_det_counts: %s", cholamd_last_error());
  const int first = tree[(1 << (L - 1)) - 1], last = tree[ns - 1]; /* labels of the first and the last leaf */
  const int a = perm[off[first - 1] + size[first - 1] / 2], e = perm[off[last - 1] + size[last - 1] / 2];
  if (run_set(p, arena, T, perm, 'A', &a, 1, &a, 1, full) || run_set(p, arena, T, perm, 'E', &a, 1, &e, 1, full) || run_set(p, arena, T, perm, 'H', all, n, all, n, full)) return 1;
  const int dup[2] = { a, a }, far[1] = { n };
  int64_t cnt[12];
  if (cholamd_plan_sparse_counts(p, dup, 2, &a, 1, cnt) != CHOLAMD_ERR_ARG || cholamd_plan_sparse_counts(p, &a, 1, far, 1, cnt) != CHOLAMD_ERR_ARG ||
      cholamd_plan_sparse_counts(p, &a, 1, &a, 1, NULL) != CHOLAMD_ERR_ARG || cholamd_plan_sparse_counts(NULL, &a, 1, &a, 1, cnt) != CHOLAMD_ERR_ARG)
    FAIL("sparse_counts accepts bad arguments");
  free(arena); free(T); free(perm); free(tree); free(off); free(size); free(all);
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
  if (cholamd_plan_sparse_solve_host_nrhs(NULL, NULL, NULL, 1, NULL, 1, -1, NULL, 1, NULL, 1, 1) != CHOLAMD_ERR_ARG) return 1;
  printf("sparse_solve_host: ok\n");
  return 0;
}
