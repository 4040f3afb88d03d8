#!/bin/bash
# A/B build of ONE translation unit of the engine for same-box measurements:
#   tools/build_ab.sh <unit> <tag> [extra hipcc flags, e.g. -DWL_STRIP_PF=3]
#   unit: main | rows | irows | strip | istrip | dtstrip | dtinv  (pytorch_wavelets_amd/csrc/wl_<unit>_hip.hip; main = wl_hip.hip)
# -> ab/libwl_<tag>.so (load with WL_LIB=ab/libwl_<tag>.so).  Every other wl_*hip.o is taken from the product build
# (python __graft_entry__.py), found by glob: a unit added to the build needs no change here.
# The numeric macros of the kernels and launchers (WL_STRIP_CWAVES, WL_STRIP_PF, WL_ROWS_DEPTH, WL_DT12_PF, ...) are what this is for.
set -e
cd "$(dirname "$0")/.."
[ $# -ge 2 ] || { echo "usage: $0 <unit> <tag> [extra hipcc flags]" >&2; exit 2; }
unit=$1; tag=$2; shift 2
C=pytorch_wavelets_amd/csrc
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
[ "$unit" = main ] && stem=wl_hip || stem=wl_${unit}_hip
[ -f $C/$stem.hip ] || { echo "no such unit: $C/$stem.hip" >&2; exit 2; }
# The per-unit compile flags are the one thing repeated here from build() of __graft_entry__.py: keep the two in step.
flags="--offload-arch=gfx950 -O3 -std=c++17 -fno-strict-aliasing -fPIC"
[ "$unit" = main ] || flags="$flags -fno-slp-vectorize -Wno-inline-asm"
[ "$unit" = dtstrip ] && flags="$flags -mllvm -pragma-unroll-threshold=100000"
others=()
for o in $C/wl_*hip.o; do
    [ "$o" = "$C/$stem.o" ] || others+=("$o")
done
nunits=$(ls $C/wl_*hip.hip | wc -l)
[ ${#others[@]} -eq $((nunits - 1)) ] || { echo "product objects missing in $C (${#others[@]} of $((nunits - 1))): run python __graft_entry__.py first" >&2; exit 1; }
mkdir -p ab
$HIPCC $flags "$@" -c $C/$stem.hip -o ab/${unit}_$tag.o
$HIPCC --offload-arch=gfx950 -shared -fPIC "${others[@]}" ab/${unit}_$tag.o -o ab/libwl_$tag.so
echo built ab/libwl_$tag.so
