/* The host side of the Schur complement (cholamd_plan_schur_size / _dofs / _list / _host) under the sanitizers, without an interpreter in the
 * process: `make asan` builds this against the sanitizer build and runs it with LeakSanitizer on.  Every k the tree allows, exact-size buffers (an
 * access past them is the sanitizer's to report), the refusals, and S = A_TT on the plain fill.  No GPU call is made. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "cholamd.h"

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

static int run_plan(cholamd_plan *p)
{
  const int L = cholamd_plan_levels(p), n = cholamd_plan_n(p);
  const int64_t na = cholamd_plan_arena_doubles(p);
  double *arena = malloc((size_t)na * sizeof(double)), *dense = malloc((size_t)n * n * sizeof(double));
  int *perm = malloc((size_t)n * sizeof(int));
  if (!arena || !dense || !perm) FAIL("out of memory");
  if (cholamd_plan_fill_host(p, arena) || cholamd_plan_arena_to_dense(p, arena, dense)) FAIL("fill: %s", cholamd_last_error());
  cholamd_plan_perm(p, perm);
  if (cholamd_plan_schur_size(p, 0) != CHOLAMD_ERR_ARG || cholamd_plan_schur_size(p, L) != CHOLAMD_ERR_ARG) FAIL("k out of range is not refused");
  if (cholamd_plan_schur_dofs(p, L, perm) != CHOLAMD_ERR_ARG || cholamd_plan_schur_list(p, 0, 0, NULL) != CHOLAMD_ERR_ARG) FAIL("k out of range is not refused");
  for (int k = 1; k <= L - 1; k++) {
    const int m = cholamd_plan_schur_size(p, k);
    if (m <= 0 || m > n) FAIL("schur_size(%d) = %d", k, m);
    int *dofs = malloc((size_t)m * sizeof(int));
    if (!dofs || cholamd_plan_schur_dofs(p, k, dofs) != m || memcmp(dofs, perm + (n - m), (size_t)m * sizeof(int))) FAIL("schur_dofs(%d)", k);
    if (cholamd_plan_schur_dofs(p, k, NULL) != CHOLAMD_ERR_ARG) FAIL("NULL dofs_out is not refused");
    const int cnt = cholamd_plan_schur_list(p, k, 0, NULL);
    if (cnt <= 0) FAIL("schur_list(%d) = %d", k, cnt);
    int64_t *rec = malloc((size_t)cnt * CHOLAMD_SCHUR_RECORD * sizeof(int64_t));
    if (!rec || cholamd_plan_schur_list(p, k, cnt, rec) != cnt) FAIL("schur_list(%d)", k);
    for (int e = 0; e < cnt; e++) { /* every record stays inside the arena and inside S */
      const int64_t *q = rec + (size_t)CHOLAMD_SCHUR_RECORD * e;
      if (q[0] < 0 || q[0] + q[2] - 1 + (q[3] - 1) * q[1] >= na || q[4] + q[2] > m || q[5] + q[3] > m || q[4] < q[5]) FAIL("record %d of k = %d", e, k);
    }
    if (cnt > 1 && cholamd_plan_schur_list(p, k, 1, rec) != cnt) FAIL("schur_list with a short buffer");
    const int64_t lds = m + 2;
    double *S = malloc((size_t)lds * m * sizeof(double));
    if (!S) FAIL("out of memory");
    for (int64_t i = 0; i < lds * m; i++) S[i] = -7.0;
    if (cholamd_plan_schur_host(p, k, arena, S, m - 1) != CHOLAMD_ERR_ARG || cholamd_plan_schur_host(p, k, NULL, S, lds) != CHOLAMD_ERR_ARG ||
        cholamd_plan_schur_host(p, k, arena, NULL, lds) != CHOLAMD_ERR_ARG)
      FAIL("schur_host accepts bad arguments");
    for (int64_t i = 0; i < lds * m; i++) if (S[i] != -7.0) FAIL("a refused schur_host wrote S");
    if (cholamd_plan_schur_host(p, k, arena, S, lds)) FAIL("schur_host: %s", cholamd_last_error());
    for (int j = 0; j < m; j++) {
      for (int i = 0; i < m; i++) { /* nothing eliminated: S = A_TT, both triangles from the stored lower one */
        const int R = n - m + (i > j ? i : j), Cc = n - m + (i > j ? j : i);
        if (S[i + j * lds] != dense[R + (size_t)Cc * n]) FAIL("S(%d, %d) of k = %d", i, j, k);
      }
      for (int64_t i = m; i < lds; i++) if (S[i + j * lds] != -7.0) FAIL("padding row %lld written", (long long)i);
    }
    free(S); free(rec); free(dofs);
  }
  free(perm); free(dense); free(arena);
  return 0;
}

int main(int argc, char **argv)
{
  if (argc < 4) { fprintf(stderr, "usage: schur_host matrix separators clusters [more triples]\n"); return 2; }
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
  if (cholamd_plan_schur_size(NULL, 1) != CHOLAMD_ERR_ARG) return 1;
  printf("schur_host: ok\n");
  return 0;
}
