#!/bin/bash
# tools/build_variant.sh <name> <file.hip> [-DMACRO=...]: _ab/lib_<name>.so = the shipped objects with <file.hip> recompiled under the given
# macros (timing / scheduling experiments, A/B on one box with tools/ab_libs.sh). Run `make -C focnerf_amd/csrc` first.
# <file.hip> may also be an edited copy elsewhere (pass -I<repo>/focnerf_amd/csrc for its includes): it replaces the object of the same name.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
name=$1; src=$2; shift 2
cd "$R/focnerf_amd/csrc"
obj=/tmp/foc_variant_${name}.o
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -Wno-unused-function -Wno-pass-failed "$@" -c "$src" -o "$obj"
# the object list is the library's own: the Makefile's SRCS
srcs=$(sed -n 's/^SRCS[[:space:]]*:=[[:space:]]*//p' Makefile)
[ -n "$srcs" ] || { echo "build_variant.sh: no SRCS in focnerf_amd/csrc/Makefile" >&2; exit 1; }
objs=""
for s in $srcs; do
  if [ "$s" = "$(basename "$src")" ]; then objs="$objs $obj"; else objs="$objs _obj/${s%.hip}.o"; fi
done
mkdir -p "$R/_ab"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$R/_ab/lib_${name}.so" $objs
echo "built $R/_ab/lib_${name}.so"
