# Builds libcholamd.so (C host code + HIP kernels for gfx950), the mmat-compatible CLI and the
# CPU oracle (test infrastructure).  No cmake needed: gcc for the C host code, hipcc for HIP.
HIPCC   ?= /opt/rocm/bin/hipcc
CC      ?= gcc
ARCH    ?= gfx950
CSRC    := cholesky_amd/csrc
OUT     := cholesky_amd/lib
BIN     := cholesky_amd/bin
CFLAGS  := -O2 -fPIC -Wall -Wextra -std=gnu11 -Iinclude -I$(CSRC)
HIPFLAGS:= -O3 -fPIC --offload-arch=$(ARCH) -Iinclude -I$(CSRC) -Wall
# the TRSM strips' step loop (trsm_rr_body, up to 20 column tiles) must unroll completely: its register tiles are indexed by the step; beyond
# LLVM's default pragma-unroll budget the loop stays rolled and the tiles go to scratch (160 B per lane).  The streamed solve needs the flag as well:
# without it the two k_solve_inv256 instances come out as different, shorter code
$(OUT)/chol_kernels.o $(OUT)/chol_solve.o: KERNFLAGS := -mllvm -pragma-unroll-threshold=100000

HOST_OBJS := $(OUT)/chol_ingest.o $(OUT)/chol_symbolic.o $(OUT)/chol_schedule.o $(OUT)/chol_lists.o $(OUT)/chol_generate.o $(OUT)/chol_lowrank_host.o $(OUT)/chol_lists_sparse.o
KERNEL_OBJS := $(OUT)/chol_kernels.o $(OUT)/chol_solve.o $(OUT)/chol_kernels_f32.o $(OUT)/chol_solve_nrhs.o $(OUT)/chol_factor_query.o $(OUT)/chol_selinv.o $(OUT)/chol_schur.o $(OUT)/chol_multiply.o $(OUT)/chol_multiply_nrhs.o $(OUT)/chol_solve_det.o $(OUT)/chol_lowrank.o $(OUT)/chol_values_grad.o $(OUT)/chol_pcg.o $(OUT)/chol_sparse.o
# the C-ABI glue: one file per family of entry points over the internal header chol_device.h
GLUE      := chol_api chol_api_factor chol_api_solve chol_api_query chol_api_pcg chol_api_schur chol_api_blas chol_api_lowrank chol_api_sparse
GLUE_HDRS := $(CSRC)/chol_device.h $(CSRC)/chol_devbuf.h $(CSRC)/chol_plan.h $(CSRC)/chol_kernels.h include/cholamd.h
GLUE_OBJS := $(GLUE:%=$(OUT)/%.o)
HIP_OBJS  := $(KERNEL_OBJS) $(GLUE_OBJS)

all: $(OUT)/libcholamd.so $(BIN)/cholamd_mmat oracle

$(OUT)/%.o: $(CSRC)/%.c $(CSRC)/chol_plan.h include/cholamd.h
	@mkdir -p $(OUT)
	$(CC) $(CFLAGS) -c $< -o $@

$(OUT)/%.o: $(CSRC)/%.hip $(CSRC)/chol_plan.h $(CSRC)/chol_kernels.h
	@mkdir -p $(OUT)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) -c $< -o $@
$(OUT)/chol_kernels.o $(OUT)/chol_solve.o: $(CSRC)/chol_wave.h

$(GLUE_OBJS): $(OUT)/%.o: $(CSRC)/%.cpp $(GLUE_HDRS)
	@mkdir -p $(OUT)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(OUT)/libcholamd.so: $(HOST_OBJS) $(HIP_OBJS)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $^ -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib

$(BIN)/cholamd_mmat: $(CSRC)/mmat_main.c $(OUT)/libcholamd.so include/cholamd.h
	@mkdir -p $(BIN)
	$(CC) $(CFLAGS) -o $@ $< -L$(OUT) -lcholamd -Wl,-rpath,'$$ORIGIN/../lib' -lm

oracle:
	$(MAKE) -s -C oracle

clean:
	rm -rf $(OUT) $(BIN)
	$(MAKE) -s -C oracle clean

.PHONY: all oracle clean

# ---- sanitizer build of the HOST code (ingest, symbolic phase, schedules, generator, C-ABI glue): AddressSanitizer +
# UBSan; the device code is built as usual (GPU sanitizers are not available on the pool).  `make asan` builds
# cholesky_amd/lib/asan/libcholamd.so and runs the CPU test-suite of the host logic against it.
ASAN_OUT := cholesky_amd/lib/asan
SAN := -fsanitize=address,undefined -fno-omit-frame-pointer -g
ASAN_HOST_OBJS := $(ASAN_OUT)/chol_ingest.o $(ASAN_OUT)/chol_symbolic.o $(ASAN_OUT)/chol_schedule.o $(ASAN_OUT)/chol_lists.o $(ASAN_OUT)/chol_generate.o $(ASAN_OUT)/chol_lowrank_host.o $(ASAN_OUT)/chol_lists_sparse.o
$(ASAN_OUT)/%.o: $(CSRC)/%.c $(CSRC)/chol_plan.h include/cholamd.h
	@mkdir -p $(ASAN_OUT)
	$(CC) $(CFLAGS) -O1 $(SAN) -c $< -o $@
$(GLUE:%=$(ASAN_OUT)/%.o): $(ASAN_OUT)/%.o: $(CSRC)/%.cpp $(GLUE_HDRS)
	@mkdir -p $(ASAN_OUT)
	$(HIPCC) $(HIPFLAGS) -O1 $(SAN) -fno-sanitize=function -fno-gpu-sanitize -x hip -c $< -o $@
$(ASAN_OUT)/libcholamd.so: $(ASAN_HOST_OBJS) $(GLUE:%=$(ASAN_OUT)/%.o) $(KERNEL_OBJS)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) $(SAN) -fno-gpu-sanitize -o $@ $^ -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
# leak detection: ON, in a process of its own without an interpreter (tests/native/host_leak.c: plans, schedules of every level and
# world size, the program builder and its self-check, the generator, error paths); the only suppression is the HIP runtime's own
# process-lifetime state (scripts/lsan.supp).  Under pytest the interpreter's and torch's allocations would drown (or, suppressed by
# frame, hide) the library's, so that run keeps detect_leaks=0.
G := tests/golden
# every tests/native/*.c program links against the sanitized library in the same way
NATIVE_PROGS := host_leak schur_host multiply_host multiply_nrhs_host solve_det_host solve_det_nrhs_host schur_solve_host lowrank_host values_grad_host pcg_host sparse_solve_host
$(NATIVE_PROGS:%=$(ASAN_OUT)/%): $(ASAN_OUT)/%: tests/native/%.c $(ASAN_OUT)/libcholamd.so
	$(HIPCC) -x c -O1 -Iinclude $(SAN) -fno-sanitize=function -o $@ $< -L$(ASAN_OUT) -lcholamd -Wl,-rpath,$(abspath $(ASAN_OUT)) -lm
# the owning device buffers of the glue over a host allocator that can be told to fail (tests/native/devbuf_host.cpp): no library, no HIP runtime
$(ASAN_OUT)/devbuf_host: tests/native/devbuf_host.cpp $(CSRC)/chol_devbuf.h
	@mkdir -p $(ASAN_OUT)
	$(HIPCC) -x c++ -O1 -I$(CSRC) $(SAN) -fno-sanitize=function -no-hip-rt -o $@ $<
ASAN_FIXTURES := $(G)/lapl_9x9/lapl_3_2.mtx $(G)/lapl_9x9/lapl_3_2_ord_2.txt $(G)/lapl_9x9/lapl_3_2_clust_2.txt \
	  $(G)/lapl_400x400/lapl_20_2.mtx $(G)/lapl_400x400/lapl_20_2_ord_5.txt $(G)/lapl_400x400/lapl_20_2_clust_5.txt \
	  $(G)/lapl_3375x3375/lapl_15_3.mtx $(G)/lapl_3375x3375/lapl_15_3_ord_5.txt $(G)/lapl_3375x3375/lapl_15_3_clust_5.txt
asan: $(ASAN_OUT)/libcholamd.so $(ASAN_OUT)/host_leak $(ASAN_OUT)/schur_host $(ASAN_OUT)/multiply_host $(ASAN_OUT)/multiply_nrhs_host $(ASAN_OUT)/solve_det_host $(ASAN_OUT)/solve_det_nrhs_host $(ASAN_OUT)/devbuf_host oracle
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 LSAN_OPTIONS=suppressions=$(abspath scripts/lsan.supp):print_suppressions=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	$(ASAN_OUT)/devbuf_host
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 LSAN_OPTIONS=suppressions=$(abspath scripts/lsan.supp):print_suppressions=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	$(ASAN_OUT)/multiply_host $(ASAN_FIXTURES) $(G)/lapl_25x25/lapl_5_2.mtx $(G)/lapl_25x25/lapl_5_2_ord_3.txt $(G)/lapl_25x25/lapl_5_2_clust_3.txt
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 LSAN_OPTIONS=suppressions=$(abspath scripts/lsan.supp):print_suppressions=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	$(ASAN_OUT)/multiply_nrhs_host $(ASAN_FIXTURES) $(G)/lapl_25x25/lapl_5_2.mtx $(G)/lapl_25x25/lapl_5_2_ord_3.txt $(G)/lapl_25x25/lapl_5_2_clust_3.txt
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 LSAN_OPTIONS=suppressions=$(abspath scripts/lsan.supp):print_suppressions=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	$(ASAN_OUT)/schur_host $(ASAN_FIXTURES)
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 LSAN_OPTIONS=suppressions=$(abspath scripts/lsan.supp):print_suppressions=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	$(ASAN_OUT)/solve_det_host $(ASAN_FIXTURES) $(G)/lapl_25x25/lapl_5_2.mtx $(G)/lapl_25x25/lapl_5_2_ord_3.txt $(G)/lapl_25x25/lapl_5_2_clust_3.txt
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 LSAN_OPTIONS=suppressions=$(abspath scripts/lsan.supp):print_suppressions=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	$(ASAN_OUT)/solve_det_nrhs_host $(ASAN_FIXTURES) $(G)/lapl_25x25/lapl_5_2.mtx $(G)/lapl_25x25/lapl_5_2_ord_3.txt $(G)/lapl_25x25/lapl_5_2_clust_3.txt
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 LSAN_OPTIONS=suppressions=$(abspath scripts/lsan.supp):print_suppressions=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	$(ASAN_OUT)/host_leak $(G)/lapl_9x9/lapl_3_2.mtx $(G)/lapl_9x9/lapl_3_2_ord_2.txt $(G)/lapl_9x9/lapl_3_2_clust_2.txt \
	  $(G)/lapl_400x400/lapl_20_2.mtx $(G)/lapl_400x400/lapl_20_2_ord_5.txt $(G)/lapl_400x400/lapl_20_2_clust_5.txt \
	  $(G)/lapl_3375x3375/lapl_15_3.mtx $(G)/lapl_3375x3375/lapl_15_3_ord_5.txt $(G)/lapl_3375x3375/lapl_15_3_clust_5.txt
	CHOLAMD_LIB=$(abspath $(ASAN_OUT)/libcholamd.so) LD_PRELOAD=$$($(CC) -print-file-name=libasan.so):$$($(CC) -print-file-name=libubsan.so) \
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 python3 -m pytest tests/test_host.py -x -q -p no:cacheprovider
.PHONY: asan
# the host restatement of the block Schur condense / expand under the sanitizers, in a process of its own (tests/native/schur_solve_host.c: it generates
# its input): `make schur_solve_host` builds and runs this program alone
schur_solve_host: $(ASAN_OUT)/schur_solve_host
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 LSAN_OPTIONS=suppressions=$(abspath scripts/lsan.supp):print_suppressions=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	$(ASAN_OUT)/schur_solve_host
.PHONY: schur_solve_host
# the host restatements of the low-rank kernels' partition under the sanitizers, in a process of its own (tests/native/lowrank_host.c: it generates its
# inputs): `make lowrank_host` builds and runs this program alone
lowrank_host: $(ASAN_OUT)/lowrank_host
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 LSAN_OPTIONS=suppressions=$(abspath scripts/lsan.supp):print_suppressions=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	$(ASAN_OUT)/lowrank_host
.PHONY: lowrank_host
# the host restatements of the values-gradient kernels under the sanitizers, in a process of its own (tests/native/values_grad_host.c: it generates its
# inputs): `make values_grad_host` builds and runs this program alone
values_grad_host: $(ASAN_OUT)/values_grad_host
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 LSAN_OPTIONS=suppressions=$(abspath scripts/lsan.supp):print_suppressions=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	$(ASAN_OUT)/values_grad_host
.PHONY: values_grad_host
# the host side of y = A x (cholamd_plan_apply_host, the operator of the PCG loop) under the sanitizers, in a process of its own (tests/native/pcg_host.c: it
# generates its inputs): `make pcg_host` builds and runs this program alone
pcg_host: $(ASAN_OUT)/pcg_host
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 LSAN_OPTIONS=suppressions=$(abspath scripts/lsan.supp):print_suppressions=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	$(ASAN_OUT)/pcg_host
.PHONY: pcg_host
# the pruned step lists of the sparse solve and their host walk (chol_lists_sparse.c) under the sanitizers, in a process of its own
# (tests/native/sparse_solve_host.c: it generates its input): `make sparse_solve_host` builds and runs this program alone
sparse_solve_host: $(ASAN_OUT)/sparse_solve_host
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 LSAN_OPTIONS=suppressions=$(abspath scripts/lsan.supp):print_suppressions=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	$(ASAN_OUT)/sparse_solve_host
.PHONY: sparse_solve_host
