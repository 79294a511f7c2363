#!/bin/bash
# Development aid: a second libcholamd.so with extra -D flags (A/B runs in one gpurun call):
#   scripts/build_alt.sh NAME [-DFOO=1 ...]   ->  cholesky_amd/lib/alt_NAME/libcholamd.so   (select with CHOLAMD_LIB=...)
# flags apply to chol_kernels.hip, chol_solve.hip, chol_kernels_f32.hip, chol_schedule.c and chol_lists.c
set -e
name=$1; shift
out=cholesky_amd/lib/alt_$name
mkdir -p $out
/opt/rocm/bin/hipcc -O3 -fPIC --offload-arch=gfx950 -Iinclude -Icholesky_amd/csrc -Wall -mllvm -pragma-unroll-threshold=100000 "$@" -c cholesky_amd/csrc/chol_kernels.hip -o $out/chol_kernels.o
/opt/rocm/bin/hipcc -O3 -fPIC --offload-arch=gfx950 -Iinclude -Icholesky_amd/csrc -Wall -mllvm -pragma-unroll-threshold=100000 "$@" -c cholesky_amd/csrc/chol_solve.hip -o $out/chol_solve.o
/opt/rocm/bin/hipcc -O3 -fPIC --offload-arch=gfx950 -Iinclude -Icholesky_amd/csrc -Wall "$@" -c cholesky_amd/csrc/chol_kernels_f32.hip -o $out/chol_kernels_f32.o
gcc -O2 -fPIC -Wall -Wextra -std=gnu11 -Iinclude -Icholesky_amd/csrc "$@" -c cholesky_amd/csrc/chol_schedule.c -o $out/chol_schedule.o
gcc -O2 -fPIC -Wall -Wextra -std=gnu11 -Iinclude -Icholesky_amd/csrc "$@" -c cholesky_amd/csrc/chol_lists.c -o $out/chol_lists.o
# every other object of the in-tree build (make first) goes in as it is
rest=$(ls cholesky_amd/lib/*.o | grep -v -e '/chol_kernels\.o$' -e '/chol_solve\.o$' -e '/chol_kernels_f32\.o$' -e '/chol_schedule\.o$' -e '/chol_lists\.o$')
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o $out/libcholamd.so $rest $out/chol_schedule.o $out/chol_lists.o $out/chol_kernels.o $out/chol_solve.o $out/chol_kernels_f32.o \
  -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
echo built $out/libcholamd.so
