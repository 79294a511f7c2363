/* cholamd_mmat -- the C driver with mmat.rg's command line (mmat.rg:1059-1093):
 *
 *   -i matrix.mtx  -s separators.txt  -c clusters.txt  [-b rhs.mtx] [-o solution] [-m factor.mtx]
 *   [-p permuted.mtx] [-d debug_dir] [--iterations n]
 * plus:  --gpu id (first device, default 0), --gpus n (subtree-sharded over n devices of this node, one RCCL all-reduce;
 *        n a power of two), --repeat n (= --iterations), --full-precision (write %.17g instead of the reference's
 *        %0.8g), --precision fp64|mixed (mixed: fp32 factor + fp64 iterative refinement of the solve),
 *        --logdet (one line "logdet: %.17g" after the factorisation: log det A = 2 sum log L_ii from the factor on the device;
 *        "logdet(fp32 factor): ..." under --precision mixed),
 *        --check (needs -b: one line "factor residual: %.3e" after the factorisation: ||A z - M M^T z|| / ||A z|| with the right-hand side as probe z and
 *        the factor of the chosen --precision applied forwards on the device, cholamd_factor_residual),
 *        --invdiag FILE (after the factorisation: diag(A^-1) by selected inversion -- cholamd_selinv + cholamd_selinv_diag -- in the solution
 *        writer's format: n lines, original dof order, %0.8g or %.17g under --full-precision; fp64 factor only),
 *        --schur K FILE (after the factorisation: the Schur complement of A on the K kept tree levels -- cholamd_schur_factor + cholamd_schur on a second,
 *        freshly filled arena -- as a Matrix-Market dense `array` file, %.17g, column by column, and the Schur dofs, 1-based, one per line, as FILE.dofs;
 *        single GPU, fp64 only),
 *        --lowrank FILE K [--lowrank-mode update|downdate|constraint] (FILE: a Matrix-Market dense `array` n x K, the columns of U; after the factorisation
 *        cholamd_lowrank_set on device 0; the solve of -b becomes the corrected solve of A + U U^T (update, the default), A - U U^T (downdate) or of A under
 *        U^T x = 0 (constraint); with --logdet one more line "logdet C: %.17g" after the logdet line: log det(A +- U U^T) = logdet + logdet C; fp64 only),
 *        --inverse-block DOFS.txt FILE (DOFS.txt: one 0-based dof per line, m of them; after the factorisation the block A^-1[S, S] of those dofs by a sparse
 *        solve of the identity -- cholamd_sparse_create + cholamd_sparse_solve_nrhs: the sweeps touch the separators of the dofs and their ancestors only --
 *        written dense in write_matrix's format: the banner, "m m m*m", then "i j value" lines, 1-based indices into the list, row by row, %0.8g or %.17g
 *        under --full-precision; fp64 factor only),
 *        --pcg (needs -b: the solve of either --precision goes through cholamd_solve_pcg / _f32 -- conjugate gradients preconditioned with the factor, 30
 *        iterations, 1e-14 -- and one stderr line "[cholamd] pcg: %d iterations, ||b - A x|| / ||b|| = %.3e", and one more with the status where that is not 0; not with --lowrank or --gpus > 1).
 * Unknown flags (the reference passes -fflow/-ll:cpu/-fcuda/-ll:csize through to Legion) are ignored.
 *
 * Flow = main() of mmat.rg:1056-1496 with the numeric phase on the GPU.  Progress lines keep the
 * reference's wording.  There is no CPU numeric path: without a HIP device the program fails.
 */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "cholamd.h"

static double now_s(void)
{
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec + 1e-9 * ts.tv_nsec;
}
#define DIE(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

int main(int argc, char **argv)
{
  const char *matrix_file = "", *separator_file = "", *clusters_file = "", *b_file = "", *solution_file = "", *factor_file = "",
             *permuted_file = "", *debug_path = "", *invdiag_file = "", *invblock_dofs = "", *invblock_file = "", *schur_file = "", *lowrank_file = "", *lowrank_mode = "update";
  int debug = 0, iterations = 1, gpu = 0, full = 0, gpus = 1, want_logdet = 0, want_check = 0, schur_k = 0, det_solve = 0, lowrank_k = 0, pcg = 0;
  const char *precision = "fp64";
  for (int i = 0; i < argc; i++) {
    const char *next = i + 1 < argc ? argv[i + 1] : "";
    if (!strcmp(argv[i], "-i")) matrix_file = next;
    else if (!strcmp(argv[i], "-s")) separator_file = next;
    else if (!strcmp(argv[i], "-c")) clusters_file = next;
    else if (!strcmp(argv[i], "-m")) factor_file = next;
    else if (!strcmp(argv[i], "-p")) permuted_file = next;
    else if (!strcmp(argv[i], "-o")) solution_file = next;
    else if (!strcmp(argv[i], "-b")) b_file = next;
    else if (!strcmp(argv[i], "-d")) { debug_path = next; debug = 1; }
    else if (!strcmp(argv[i], "--iterations")) iterations = atoi(next);
    else if (!strcmp(argv[i], "--repeat")) iterations = atoi(next);
    else if (!strcmp(argv[i], "--gpu")) gpu = atoi(next);
    else if (!strcmp(argv[i], "--gpus")) gpus = atoi(next);
    else if (!strcmp(argv[i], "--precision")) precision = next;
    else if (!strcmp(argv[i], "--full-precision")) full = 1;
    else if (!strcmp(argv[i], "--logdet")) want_logdet = 1;
    else if (!strcmp(argv[i], "--check")) want_check = 1;
    else if (!strcmp(argv[i], "--deterministic-solve")) det_solve = 1; /* device option solve_deterministic for the solve of -b: the same bits in every run */
    else if (!strcmp(argv[i], "--pcg")) pcg = 1;
    else if (!strcmp(argv[i], "--invdiag")) invdiag_file = next;
    else if (!strcmp(argv[i], "--inverse-block")) { invblock_dofs = next; invblock_file = i + 2 < argc ? argv[i + 2] : ""; if (!*invblock_dofs || !*invblock_file) DIE("--inverse-block DOFS.txt FILE"); }
    else if (!strcmp(argv[i], "--schur")) { schur_k = atoi(next); schur_file = i + 2 < argc ? argv[i + 2] : ""; if (!*schur_file) DIE("--schur K FILE"); }
    else if (!strcmp(argv[i], "--lowrank")) { lowrank_file = next; lowrank_k = i + 2 < argc ? atoi(argv[i + 2]) : 0; if (!*lowrank_file || lowrank_k < 1) DIE("--lowrank FILE K"); }
    else if (!strcmp(argv[i], "--lowrank-mode")) lowrank_mode = next;
  }
  printf("Iterations: %d\n", iterations);
  if (!*matrix_file || !*separator_file || !*clusters_file) DIE("usage: %s -i A.mtx -s ord.txt -c clust.txt [-b B.mtx -o x.txt] [-m L.mtx] [-p PAPt.mtx] [-d dir] [--iterations n]", argv[0]);

  double t0 = now_s();
  cholamd_plan *plan = NULL;
  if (cholamd_plan_create(matrix_file, separator_file, clusters_file, &plan)) DIE("plan: %s", cholamd_last_error());
  const int n = cholamd_plan_n(plan), levels = cholamd_plan_levels(plan);
  printf("M: %d N: %d nz: %d typecode: %s\n", n, n, cholamd_plan_nz(plan), cholamd_plan_banner(plan));
  printf("levels: %d\nseparators: %d\nMax Interval Size: %d\n", levels, cholamd_plan_num_separators(plan), cholamd_plan_max_int_size(plan));
  printf("Blocks ispace: %d\n", cholamd_plan_num_blocks(plan));
  if (cholamd_plan_dropped_entries(plan))
    fprintf(stderr, "warning: %ld matrix entries lie outside every ancestor/descendant block and were dropped\n", (long)cholamd_plan_dropped_entries(plan));
  double t_sym = now_s() - t0;

  const int64_t na = cholamd_plan_arena_doubles(plan);
  double *h_arena = malloc((size_t)na * sizeof(double));
  if (!h_arena) DIE("out of memory");
  if (*permuted_file) { /* mmat.rg:1187-1189 */
    cholamd_plan_fill_host(plan, h_arena);
    printf("saving matrix to: %s\n\n", permuted_file);
    if (cholamd_plan_write_matrix(plan, h_arena, permuted_file, full)) DIE("%s", cholamd_last_error());
  }
  if (debug) { /* Block / Cluster / Fill lines of the symbolic phase on stdout, where verify.debug_factor's log comes from */
    if (gpus > 1 || !strcmp(precision, "mixed")) DIE("-d (debug mode) is a single-GPU fp64 path");
    cholamd_plan_write_debug_header(plan, stdout);
  }

  const int mixed = !strcmp(precision, "mixed");
  if (!mixed && strcmp(precision, "fp64")) DIE("--precision %s: fp64 or mixed", precision);
  if (mixed && gpus > 1) DIE("--precision mixed is a single-GPU path");
  if (want_check && !*b_file) DIE("--check takes the right-hand side as its probe: it needs -b");
  if (mixed && *invdiag_file) DIE("--invdiag needs the fp64 factor (--precision fp64)");
  if (mixed && *invblock_file) DIE("--inverse-block needs the fp64 factor (--precision fp64)");
  int *invblock_list = NULL, invblock_m = 0;
  if (*invblock_file) { /* the list is read before any device work; the library names a dof that is out of range or listed twice */
    FILE *fd = fopen(invblock_dofs, "r");
    if (!fd) DIE("cannot read %s", invblock_dofs);
    int v = 0, more = 0;
    invblock_list = malloc((size_t)(n > 0 ? n : 1) * sizeof(int));
    if (!invblock_list) DIE("out of memory");
    while (fscanf(fd, "%d", &v) == 1) { if (invblock_m < n) invblock_list[invblock_m++] = v; else more = 1; }
    fclose(fd);
    if (invblock_m < 1 || more) DIE("--inverse-block: %s holds %s", invblock_dofs, more ? "more dofs than the matrix has" : "no dof");
  }
  if (*schur_file && (mixed || gpus > 1)) DIE("--schur is a single-GPU fp64 path");
  if (*schur_file && cholamd_plan_schur_size(plan, schur_k) < 0) DIE("--schur: %s", cholamd_last_error());
  const int lr_mode = !strcmp(lowrank_mode, "update") ? CHOLAMD_LOWRANK_UPDATE : !strcmp(lowrank_mode, "downdate") ? CHOLAMD_LOWRANK_DOWNDATE : CHOLAMD_LOWRANK_CONSTRAINT;
  if (*lowrank_file && mixed) DIE("--lowrank needs the fp64 factor (--precision fp64)");
  if (pcg && *lowrank_file) DIE("--pcg does not take a low-rank object (--lowrank)");
  if (pcg && !*b_file) DIE("--pcg is a form of the solve: it needs -b");
  if (pcg && gpus > 1) DIE("--pcg is a single-GPU path");
  if (*lowrank_file && lr_mode == CHOLAMD_LOWRANK_CONSTRAINT && strcmp(lowrank_mode, "constraint")) DIE("--lowrank-mode %s: update, downdate or constraint", lowrank_mode);
  if (*lowrank_file && (lowrank_k > CHOLAMD_LOWRANK_MAX || (int64_t)n * lowrank_k > 2147483647)) DIE("--lowrank: K = %d (at most %d, and n K must fit an int)", lowrank_k, CHOLAMD_LOWRANK_MAX);
  if (gpus < 1 || gpus > 64 || (gpus & (gpus - 1))) DIE("--gpus must be a power of two");
  if (cholamd_device_count() < gpu + gpus) DIE("--gpus %d from device %d: only %d HIP devices are visible", gpus, gpu, cholamd_device_count());
  /* one device object + arena per GPU; devs[0] ends up with the complete factor */
  cholamd_device *devs[64] = { NULL };
  double *arenas[64] = { NULL };
  cholamd_comm *comms[64] = { NULL };
  for (int g = 0; g < gpus; g++) {
    if (cholamd_device_create(plan, gpu + g, &devs[g])) DIE("device %d: %s", gpu + g, cholamd_last_error());
    if (gpus > 1 && cholamd_device_set_partition(devs[g], g, gpus)) DIE("partition: %s", cholamd_last_error());
    if (cholamd_device_alloc(devs[g], na, &arenas[g])) DIE("alloc: %s", cholamd_last_error());
  }
  if (gpus > 1 && cholamd_comm_create_all(devs, gpus, comms)) DIE("rccl: %s", cholamd_last_error());
  cholamd_device *dev = devs[0];
  double *d_arena = arenas[0];
  if (det_solve && cholamd_device_set_option(dev, "solve_deterministic", 1)) DIE("--deterministic-solve: %s", cholamd_last_error());
  printf("Done fill.\n");
  double t_factor = 0;
  for (int it = 0; it < iterations; it++) { /* mmat.rg:1212-1358 */
    for (int g = 0; g < gpus; g++)
      if ((mixed ? cholamd_device_fill_f32(devs[g], (float *)arenas[g], NULL) : cholamd_device_fill(devs[g], arenas[g], NULL)) || cholamd_device_sync(devs[g], NULL)) DIE("fill: %s", cholamd_last_error());
    for (int lvl = levels - 1, interval = 0; lvl >= 0; lvl--) {
      printf("Factoring Level: %d Interval: %d Iteration: %d\n", lvl, interval, it);
      if (lvl <= levels - 2) interval++;
    }
    double t1 = now_s();
    if (debug) { /* one fused task at a time, op lines on stdout, write_blocks dumps in debug_path (mmat.rg:1255,1288,1342) */
      if (cholamd_factor_debug(dev, d_arena, debug_path, full, NULL)) DIE("factor (debug): %s", cholamd_last_error());
    } else
    if (mixed ? cholamd_factor_f32(dev, (float *)d_arena, NULL) : cholamd_factor_multi(devs, arenas, comms, gpus, NULL)) DIE("factor: %s", cholamd_last_error());
    for (int g = 0; g < gpus; g++) if (cholamd_device_sync(devs[g], NULL)) DIE("factor: %s", cholamd_last_error());
    t_factor = now_s() - t1;
    for (int g = 0; g < gpus; g++) {
      int sep = 0, info = cholamd_factor_info(devs[g], &sep);
      if (info < 0) DIE("factor: %s", cholamd_last_error()); /* internal failure (stall watchdog / HIP error): no output file is written */
      if (info > 0) fprintf(stderr, "warning: leading minor %d of separator %d is not positive definite\n", info, sep);
    }
    printf("Done factoring Iteration: %d.\n", it);
  }
  if (gpus > 1) { /* the subtrees' panels -> device 0 */
    if (cholamd_gather_factor(devs, arenas, gpus, NULL) || cholamd_device_sync(dev, NULL)) DIE("gather: %s", cholamd_last_error());
  }
  const double flops = cholamd_plan_flops(plan);
  fprintf(stderr, "[cholamd] %d GPU(s), symbolic %.3f ms, numeric factorisation %.3f ms, F_ref %.6g flop, %.3f GF/s, B_alg %ld bytes\n",
          gpus, 1e3 * t_sym, 1e3 * t_factor, flops, flops / t_factor * 1e-9, (long)cholamd_plan_alg_bytes(plan));

  cholamd_lowrank *lr = NULL;
  if (*lowrank_file) { /* the complete factor is on device 0 */
    const int64_t nk = (int64_t)n * lowrank_k;
    double *U = malloc((size_t)nk * sizeof(double)), *d_U = NULL;
    if (!U) DIE("out of memory");
    if (cholamd_read_vector(lowrank_file, (int)nk, U)) DIE("%s", cholamd_last_error());
    if (cholamd_device_alloc(dev, nk, &d_U) || cholamd_device_upload(dev, d_U, U, nk, NULL)) DIE("%s", cholamd_last_error());
    if (cholamd_lowrank_create(dev, lowrank_k, &lr) || cholamd_lowrank_set(lr, d_arena, d_U, n, lowrank_k, lr_mode, NULL)) DIE("lowrank: %s", cholamd_last_error());
    cholamd_device_free(dev, d_U);
    free(U);
  }
  if (want_logdet) { /* the complete factor is on device 0 */
    double logdet = 0.0;
    if (mixed ? cholamd_factor_logdet_f32(dev, (const float *)d_arena, &logdet, NULL) : cholamd_factor_logdet(dev, d_arena, &logdet, NULL)) DIE("logdet: %s", cholamd_last_error());
    printf(mixed ? "logdet(fp32 factor): %.17g\n" : "logdet: %.17g\n", logdet);
    if (lr) {
      double logdet_c = 0.0;
      if (cholamd_lowrank_logdet(lr, &logdet_c)) DIE("lowrank: %s", cholamd_last_error());
      printf("logdet C: %.17g\n", logdet_c);
    }
  }
  if (want_check) { /* the complete factor is on device 0; the probe is the right-hand side */
    double *z = malloc((size_t)n * sizeof(double)), *d_z = NULL, rel = 0.0;
    if (!z) DIE("out of memory");
    if (cholamd_read_vector(b_file, n, z)) DIE("%s", cholamd_last_error());
    if (cholamd_device_alloc(dev, n, &d_z) || cholamd_device_upload(dev, d_z, z, n, NULL)) DIE("%s", cholamd_last_error());
    if (mixed ? cholamd_factor_residual_f32(dev, (const float *)d_arena, d_z, &rel, NULL) : cholamd_factor_residual(dev, d_arena, d_z, &rel, NULL)) DIE("check: %s", cholamd_last_error());
    printf("factor residual: %.3e\n", rel);
    cholamd_device_free(dev, d_z);
    free(z);
  }
  if (*invdiag_file) { /* the complete factor is on device 0; the Z arena is a second arena */
    double *d_z = NULL, *d_diag = NULL, *diag = malloc((size_t)n * sizeof(double));
    if (!diag) DIE("out of memory");
    if (cholamd_device_alloc(dev, na, &d_z) || cholamd_device_alloc(dev, n, &d_diag)) DIE("alloc: %s", cholamd_last_error());
    if (cholamd_selinv(dev, d_arena, d_z, NULL) || cholamd_selinv_diag(dev, d_z, d_diag, NULL) || cholamd_device_download(dev, diag, d_diag, n, NULL))
      DIE("invdiag: %s", cholamd_last_error());
    printf("Saving diagonal of the inverse to: %s\n", invdiag_file);
    if (cholamd_write_solution(invdiag_file, diag, n, full)) DIE("%s", cholamd_last_error());
    cholamd_device_free(dev, d_z); cholamd_device_free(dev, d_diag);
    free(diag);
  }
  if (*invblock_file) { /* the complete factor is on device 0; the identity is solved in place */
    const int m = invblock_m;
    int *dofs = invblock_list;
    const int64_t mm = (int64_t)m * m;
    double *Z = calloc((size_t)mm, sizeof(double)), *d_Z = NULL;
    if (!Z) DIE("out of memory");
    for (int i = 0; i < m; i++) Z[i + (size_t)i * m] = 1.0;
    cholamd_sparse *sp = NULL;
    if (cholamd_sparse_create(dev, dofs, m, dofs, m, &sp)) DIE("inverse-block: %s", cholamd_last_error());
    if (cholamd_device_alloc(dev, mm, &d_Z) || cholamd_device_upload(dev, d_Z, Z, mm, NULL)) DIE("%s", cholamd_last_error());
    if (cholamd_sparse_solve_nrhs(sp, d_arena, d_Z, m, d_Z, m, m, -1, NULL) || cholamd_device_download(dev, Z, d_Z, mm, NULL)) DIE("inverse-block: %s", cholamd_last_error());
    printf("Saving inverse block (%d dofs) to: %s\n", m, invblock_file);
    FILE *fz = fopen(invblock_file, "w");
    if (!fz) DIE("cannot write %s", invblock_file);
    fprintf(fz, "%%%%MatrixMarket matrix coordinate real general\n%d %d %lld\n", m, m, (long long)mm);
    for (int i = 0; i < m; i++)
      for (int j = 0; j < m; j++) fprintf(fz, full ? "%d %d %.17g\n" : "%d %d %0.8g\n", i + 1, j + 1, Z[i + (size_t)j * m]);
    if (fclose(fz)) DIE("cannot write %s", invblock_file);
    cholamd_sparse_destroy(sp);
    cholamd_device_free(dev, d_Z);
    free(Z); free(dofs);
  }
  if (*schur_file) { /* a second arena, filled again and eliminated down to level K only: its kept blocks hold S */
    const int m = cholamd_plan_schur_size(plan, schur_k);
    double *d_a2 = NULL, *d_S = NULL, *S = malloc((size_t)(m > 0 ? m : 1) * (size_t)(m > 0 ? m : 1) * sizeof(double));
    int *dofs = malloc((size_t)(m > 0 ? m : 1) * sizeof(int));
    if (!S || !dofs) DIE("out of memory");
    if (cholamd_device_alloc(dev, na, &d_a2) || cholamd_device_alloc(dev, (int64_t)(m > 0 ? m : 1) * (m > 0 ? m : 1), &d_S)) DIE("alloc: %s", cholamd_last_error());
    if (cholamd_device_fill(dev, d_a2, NULL) || cholamd_schur_factor(dev, d_a2, schur_k, NULL) || cholamd_schur(dev, d_a2, schur_k, d_S, m, NULL) ||
        cholamd_device_download(dev, S, d_S, (int64_t)m * m, NULL) || cholamd_plan_schur_dofs(plan, schur_k, dofs) < 0)
      DIE("schur: %s", cholamd_last_error());
    int sep = 0, info = cholamd_factor_info(dev, &sep);
    if (info < 0) DIE("schur: %s", cholamd_last_error());
    if (info > 0) fprintf(stderr, "warning: leading minor %d of separator %d is not positive definite\n", info, sep);
    printf("Saving Schur complement (%d kept levels, %d dofs) to: %s\n", schur_k, m, schur_file);
    FILE *fs = fopen(schur_file, "w");
    if (!fs) DIE("cannot write %s", schur_file);
    fprintf(fs, "%%%%MatrixMarket matrix array real general\n%d %d\n", m, m);
    for (int64_t e = 0; e < (int64_t)m * m; e++) fprintf(fs, "%.17g\n", S[e]);
    if (fclose(fs)) DIE("cannot write %s", schur_file);
    char *dofs_name = malloc(strlen(schur_file) + 6);
    if (!dofs_name) DIE("out of memory");
    sprintf(dofs_name, "%s.dofs", schur_file);
    FILE *fd = fopen(dofs_name, "w");
    if (!fd) DIE("cannot write %s", dofs_name);
    for (int i = 0; i < m; i++) fprintf(fd, "%d\n", dofs[i] + 1);
    if (fclose(fd)) DIE("cannot write %s", dofs_name);
    cholamd_device_free(dev, d_a2); cholamd_device_free(dev, d_S);
    free(dofs_name); free(dofs); free(S);
  }
  if (*factor_file) { /* mmat.rg:1360-1362 */
    if (cholamd_device_download(dev, h_arena, d_arena, na, NULL)) DIE("download: %s", cholamd_last_error());
    if (mixed) { /* the device arena holds na floats (in the first half of the buffer): widen in place, back to front */
      const float *f = (const float *)h_arena;
      for (int64_t i = na - 1; i >= 0; i--) h_arena[i] = (double)f[i];
    }
    printf("saving matrix to: %s\n\n", factor_file);
    if (cholamd_plan_write_matrix(plan, h_arena, factor_file, full)) DIE("%s", cholamd_last_error());
  }
  if (*b_file) { /* mmat.rg:1364-1495 */
    double *b = malloc((size_t)n * sizeof(double)), *x = malloc((size_t)n * sizeof(double)), *d_b = NULL, *d_x = NULL;
    if (cholamd_read_vector(b_file, n, b)) DIE("%s", cholamd_last_error());
    if (cholamd_device_alloc(dev, n, &d_b) || cholamd_device_alloc(dev, n, &d_x) || cholamd_device_upload(dev, d_b, b, n, NULL)) DIE("%s", cholamd_last_error());
    printf("Forward Substitution\nBackward Substitution\n");
    if (pcg) {
      int iters = 0, status = 0; double rel = 0.0;
      if (mixed ? cholamd_solve_pcg_f32(dev, (const float *)d_arena, d_b, d_x, 30, 1e-14, 0, &iters, &rel, &status, NULL)
                : cholamd_solve_pcg(dev, d_arena, d_b, d_x, 30, 1e-14, 0, &iters, &rel, &status, NULL)) DIE("solve: %s", cholamd_last_error());
      fprintf(stderr, "[cholamd] pcg: %d iterations, ||b - A x|| / ||b|| = %.3e\n", iters, rel);
      if (status) fprintf(stderr, "[cholamd] pcg: status %d, not converged to 1e-14 in 30 iterations\n", status);
      if (cholamd_device_download(dev, x, d_x, n, NULL)) DIE("solve: %s", cholamd_last_error());
    } else if (mixed) {
      int iters = 0; double rel = 0.0;
      if (cholamd_solve_refine(dev, (const float *)d_arena, d_b, d_x, 30, 1e-14, &iters, &rel, NULL)) DIE("solve: %s", cholamd_last_error());
      fprintf(stderr, "[cholamd] iterative refinement: %d corrections, ||b - A x|| / ||b|| = %.3e\n", iters, rel);
      if (cholamd_device_download(dev, x, d_x, n, NULL)) DIE("solve: %s", cholamd_last_error());
    } else if ((lr ? cholamd_lowrank_solve(lr, d_arena, d_b, NULL, d_x, NULL) : cholamd_solve(dev, d_arena, d_b, d_x, NULL)) || cholamd_device_download(dev, x, d_x, n, NULL)) DIE("solve: %s", cholamd_last_error());
    printf("Done solve.\n");
    if (*solution_file) {
      printf("Saving solution to: %s\n", solution_file);
      if (cholamd_write_solution(solution_file, x, n, full)) DIE("%s", cholamd_last_error());
    }
    cholamd_device_free(dev, d_b); cholamd_device_free(dev, d_x);
    free(b); free(x);
  }
  cholamd_lowrank_destroy(lr);
  for (int g = 0; g < gpus; g++) {
    cholamd_comm_destroy(comms[g]);
    cholamd_device_free(devs[g], arenas[g]);
    cholamd_device_destroy(devs[g]);
  }
  cholamd_plan_destroy(plan);
  free(h_arena);
  return 0;
}
