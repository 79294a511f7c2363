/* The host restatements of the low-rank kernels' partition (cholamd_lowrank_slabs, cholamd_lowrank_tprod_host, cholamd_lowrank_rprod_host) under the
 * sanitizers, without an interpreter in the process: `make lowrank_host` builds this against the sanitizer build and runs it with LeakSanitizer on.  It
 * generates its own inputs, walks the sizes at the slab boundaries with exact-size buffers (an access past them is the sanitizer's to report), checks the
 * results against plain loops within the inner-product bounds, the in-place product, and the refusals.  No GPU call. */
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

static int run(int64_t n, int k, int m)
{
  const int64_t ldp = n > 0 ? n : 1, ldt = k;
  double *P = gen(ldp * k, 0.37), *Q = gen(ldp * m, 0.11), *T = gen((int64_t)k * m, 0.5), *X = gen(ldp * m, 0.23), *X0 = gen(ldp * m, 0.23), *R = gen((int64_t)k * k, 0.7);
  if (!P || !Q || !T || !X || !X0 || !R) FAIL("out of memory");
  if (cholamd_lowrank_tprod_host(n, k, m, P, ldp, Q, ldp, T, ldt)) FAIL("tprod: %s", cholamd_last_error());
  for (int j = 0; j < m; j++)
    for (int i = 0; i < k; i++) {
      double ref = 0.0, mag = 0.0;
      for (int64_t r = 0; r < n; r++) { ref += P[r + i * ldp] * Q[r + j * ldp]; mag += fabs(P[r + i * ldp] * Q[r + j * ldp]); }
      if (!(fabs(T[i + j * ldt] - ref) <= 2.0 * (double)(n + 2) * U * mag)) FAIL("tprod n = %lld k = %d m = %d: T(%d, %d) = %.17g, plain loop %.17g", (long long)n, k, m, i, j, T[i + j * ldt], ref);
    }
  if (cholamd_lowrank_rprod_host(n, k, m, 0.5, -2.0, P, ldp, T, ldt, X, ldp)) FAIL("rprod: %s", cholamd_last_error());
  for (int j = 0; j < m; j++)
    for (int64_t r = 0; r < n; r++) {
      double ref = 0.0, mag = 0.0;
      for (int c = 0; c < k; c++) { ref += P[r + c * ldp] * T[c + j * ldt]; mag += fabs(P[r + c * ldp] * T[c + j * ldt]); }
      ref = 0.5 * X0[r + j * ldp] - 2.0 * ref; mag = 0.5 * fabs(X0[r + j * ldp]) + 2.0 * mag;
      if (!(fabs(X[r + j * ldp] - ref) <= 2.0 * (double)(k + 3) * U * mag)) FAIL("rprod n = %lld k = %d m = %d: X(%lld, %d) = %.17g, plain loop %.17g", (long long)n, k, m, (long long)r, j, X[r + j * ldp], ref);
    }
  /* in place: P <- P R equals the out-of-place product bit for bit */
  double *Y = gen(ldp * k, 0.0), *Pc = gen(ldp * k, 0.37);
  if (!Y || !Pc) FAIL("out of memory");
  if (cholamd_lowrank_rprod_host(n, k, k, 0.0, 1.0, P, ldp, R, k, Y, ldp) || cholamd_lowrank_rprod_host(n, k, k, 0.0, 1.0, Pc, ldp, R, k, Pc, ldp)) FAIL("rprod in place: %s", cholamd_last_error());
  for (int c = 0; c < k; c++) if (n > 0 && memcmp(Y + c * ldp, Pc + c * ldp, (size_t)n * sizeof(double))) FAIL("rprod in place differs in column %d (n = %lld, k = %d)", c, (long long)n, k);
  free(P); free(Q); free(T); free(X); free(X0); free(R); free(Y); free(Pc);
  return 0;
}

int main(void)
{
  const int64_t S = cholamd_lowrank_slabs(1, NULL, 0) == 1 ? 1024 : -1; /* CHOL_LR_SLAB */
  if (cholamd_lowrank_slabs(S, NULL, 0) != 1 || cholamd_lowrank_slabs(S + 1, NULL, 0) != 2) FAIL("the slab size is not %lld", (long long)S);
  const int64_t sizes[] = { 0, 1, 15, 16, 17, S - 1, S, S + 1, 2 * S - 1, 2 * S + 1, 3375 };
  for (size_t q = 0; q < sizeof sizes / sizeof *sizes; q++) {
    const int64_t n = sizes[q];
    const int ns = cholamd_lowrank_slabs(n, NULL, 0);
    if (ns != (int)((n + S - 1) / S)) FAIL("slabs(%lld) = %d", (long long)n, ns);
    int64_t *first = malloc((size_t)(ns > 0 ? ns : 1) * sizeof(int64_t));
    if (!first) FAIL("out of memory");
    if (cholamd_lowrank_slabs(n, first, ns) != ns) FAIL("slabs(%lld) with a buffer", (long long)n);
    for (int s = 0; s < ns; s++) if (first[s] != s * S || first[s] >= n) FAIL("slab %d of n = %lld starts at %lld", s, (long long)n, (long long)first[s]);
    free(first);
    const int ks[] = { 1, 17, 33 }, ms[] = { 1, 33, 5 };
    for (int c = 0; c < 3; c++) if (run(n, ks[c], ms[c])) return 1;
  }
  if (run(300, 256, 32)) return 1;
  /* refusals: nothing is written */
  double a[4] = { 1, 2, 3, 4 }, t[4] = { 9, 9, 9, 9 };
  if (cholamd_lowrank_slabs(-1, NULL, 0) != CHOLAMD_ERR_ARG) FAIL("slabs accepts n < 0");
  if (cholamd_lowrank_tprod_host(2, 2, 2, a, 1, a, 2, t, 2) != CHOLAMD_ERR_ARG || cholamd_lowrank_tprod_host(2, 2, 2, a, 2, a, 2, t, 1) != CHOLAMD_ERR_ARG ||
      cholamd_lowrank_tprod_host(2, 257, 1, a, 2, a, 2, t, 257) != CHOLAMD_ERR_ARG || cholamd_lowrank_tprod_host(2, 2, 2, NULL, 2, a, 2, t, 2) != CHOLAMD_ERR_ARG ||
      cholamd_lowrank_tprod_host(-1, 2, 2, a, 2, a, 2, t, 2) != CHOLAMD_ERR_ARG || cholamd_lowrank_tprod_host(2, 2, 2, a, 2, a, 2, NULL, 2) != CHOLAMD_ERR_ARG)
    FAIL("tprod_host accepts bad arguments");
  if (cholamd_lowrank_rprod_host(2, 2, 2, 0.0, 1.0, a, 1, a, 2, t, 2) != CHOLAMD_ERR_ARG || cholamd_lowrank_rprod_host(2, 2, 2, 0.0, 1.0, a, 2, a, 1, t, 2) != CHOLAMD_ERR_ARG ||
      cholamd_lowrank_rprod_host(2, 2, 2, 0.0, 1.0, a, 2, a, 2, t, 1) != CHOLAMD_ERR_ARG || cholamd_lowrank_rprod_host(2, 2, 2, 0.0, 1.0, a, 2, NULL, 2, t, 2) != CHOLAMD_ERR_ARG)
    FAIL("rprod_host accepts bad arguments");
  for (int i = 0; i < 4; i++) if (t[i] != 9) FAIL("a refused call wrote its output");
  if (cholamd_lowrank_tprod_host(2, 0, 2, a, 2, a, 2, t, 1) || cholamd_lowrank_rprod_host(2, 2, 0, 0.0, 1.0, a, 2, a, 2, t, 2)) FAIL("k == 0 / m == 0 must return 0");
  for (int i = 0; i < 4; i++) if (t[i] != 9) FAIL("an empty call wrote its output");
  printf("lowrank_host ok\n");
  return 0;
}
