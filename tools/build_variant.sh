#!/bin/bash
# usage: tools/build_variant.sh <name: a source of the library without .hip, e.g. chess|decimate|cc|preprocess> <variant.hip> <out.so> [extra flags]
# Links the library with <variant.hip> in the place of csrc/<name>.hip (the other objects as `make` builds them).
set -e
R=$(cd $(dirname $0)/.. && pwd)
NAME=$1; SRC=$2; OUT=$3; shift 3
B=$R/mrgingham_amd/csrc/build
make -s -C $R/mrgingham_amd/csrc -j4 all >/dev/null
cp $SRC $R/mrgingham_amd/csrc/_variant_$NAME.hip
EXTRA=""; [ "$NAME" = chess ] && EXTRA="-mllvm -amdgpu-sched-strategy=max-ilp"
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=off -Wno-unused-value -DMRG_EXPERIMENT $EXTRA "$@" -c $R/mrgingham_amd/csrc/_variant_$NAME.hip -o /tmp/_variant_$NAME.o
rm -f $R/mrgingham_amd/csrc/_variant_$NAME.hip
OBJS=""
for n in $(make -s -C $R/mrgingham_amd/csrc print-srcs); do n=${n%.hip}; if [ $n = $NAME ]; then OBJS="$OBJS /tmp/_variant_$NAME.o"; else OBJS="$OBJS $B/$n.o"; fi; done
for n in $(make -s -C $R/mrgingham_amd/csrc print-host-srcs); do OBJS="$OBJS $B/${n%.cpp}.o"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT $OBJS $B/grid.o -lz -ldl
echo built $OUT
