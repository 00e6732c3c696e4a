#!/bin/bash
# Build profiling variants of libmosaic_gpu.so: tools/variants.sh NAME "-DFOO=1" [NAME "-D..."]...
# Each lands in build/ab/NAME/libmosaic_gpu.so (select with MOSAIC_AMD_LIB).  The
# variants' kernels.hip compiles run in parallel; the host objects are the tree's.
set -e
cd "$(dirname "$0")/../mosaic_amd/csrc"
make -s
CXXFLAGS="-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wno-unused-result -Wno-unused-value"
# the objects of one variant: the tree's (Makefile OBJ), with the ones it rebuilds taken from its directory
HIPCC=/opt/rocm/bin/hipcc
link() {  # link DIR REBUILT_OBJECT...
  local d=$1 objs=" kernels.o capi.o chip_build.o comm.o tessellate.o bng_format.o h3_glibc.o ring_join.o geom_kernels.o cell_agg.o "
  shift
  for o in "$@"; do objs=${objs/ $o / $d/$o }; done
  $HIPCC --offload-arch=gfx950 -shared -o $d/libmosaic_gpu.so $objs -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib &&
    (cd $d && rm -f "$@")
}
pids=()
names=()
while [ $# -ge 2 ]; do
  d=../../build/ab/$1; mkdir -p $d
  if [ "${2#all:}" != "$2" ]; then  # NAME "all:-D..." rebuilds kernels.hip and both host files (capi.cpp, chip_build.cpp) with the flags
    ($HIPCC $CXXFLAGS ${2#all:} -c capi.cpp -o $d/capi.o 2> $d/build.log &&
     $HIPCC $CXXFLAGS ${2#all:} -c chip_build.cpp -o $d/chip_build.o 2>> $d/build.log &&
     $HIPCC --offload-arch=gfx950 $CXXFLAGS ${2#all:} -c kernels.hip -o $d/kernels.o 2>> $d/build.log &&
     link $d kernels.o capi.o chip_build.o) &
  elif [ "${2#host:}" != "$2" ]; then  # NAME "host:-D..." rebuilds chip_build.cpp (the chip-table builder) instead
    ($HIPCC $CXXFLAGS ${2#host:} -c chip_build.cpp -o $d/chip_build.o 2> $d/build.log &&
     link $d chip_build.o) &
  else
    ($HIPCC --offload-arch=gfx950 $CXXFLAGS $2 -c kernels.hip -o $d/kernels.o 2> $d/build.log &&
     link $d kernels.o) &
  fi
  pids+=($!); names+=($1)
  shift 2
done
for i in "${!pids[@]}"; do wait ${pids[$i]} || { echo "variant ${names[$i]} failed"; exit 1; }; done
