#!/bin/bash
# Dev tool: build a tuning variant of ONE kernel set (default (16,0)) into scratch: tools/variants/<name>.so
#   [NR=64 NC=0 DENSE=1 PER_CHAIN=0] tools/build_variant.sh <name> <extra hipcc flags...>
# and select it with METROPOLIS_HIP_LIB=tools/variants/<name>.so
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p tools/variants/obj_$name
hip="hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I include"
# the dimension-independent units, each with the flags build.py gives it
while read -r unit flags; do
  $hip $flags "$@" -c metropolisengine_amd/csrc/$unit.hip -o tools/variants/obj_$name/$unit.o &
done < <(python -c "from metropolisengine_amd import build; [print(unit, *flags) for unit, flags in build.HOST_UNITS]")
$hip -DME_NR=${NR:-16} -DME_NC=${NC:-0} -DME_DENSE=${DENSE:-0} -DME_PER_CHAIN=${PER_CHAIN:-1} "$@" \
  -c metropolisengine_amd/csrc/me_kernels.hip -o tools/variants/obj_$name/k.o &
wait
hipcc --offload-arch=gfx950 -shared -fPIC -o tools/variants/$name.so tools/variants/obj_$name/*.o
echo built tools/variants/$name.so
