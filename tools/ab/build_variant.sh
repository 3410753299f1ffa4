#!/bin/bash
# A/B builds of the library: tools/ab/build_variant.sh <tag> "<-D flags>"
# -> opencl-raytracer_amd/csrc/variants/libhip_raytracer_<tag>.so (git-ignored, travels with gpurun).
# Load one with RT_LIB_OVERRIDE=<path> (hip_raytracer.load_library).
# Same units and flags as the Makefile (its SRCS list is read, not copied); JOBS compilers at a time (default 8).
set -e
cd "$(dirname "$0")/../../opencl-raytracer_amd/csrc"
tag=$1; defs=$2
[ -n "$tag" ] || { echo "usage: $0 <tag> \"<-D flags>\"" >&2; exit 2; }
mkdir -p variants
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math -I../../include -I. $defs"
srcs=$(sed -n '/^SRCS/,/^HDRS/p' Makefile | grep -o 'rt_[a-z_]*\.\(hip\|cpp\)')
[ -n "$srcs" ] || { echo "no sources found in the Makefile" >&2; exit 1; }
objs=""
for f in $srcs; do objs="$objs variants/${f%.*}_$tag.o"; done
one() {  # <source>: one unit; .cpp units are HIP too (the Makefile's -x hip)
    local f=$1 x=""
    case $f in *.cpp) x="-x hip";; esac
    /opt/rocm/bin/hipcc $FLAGS $x -c "$f" -o "variants/${f%.*}_$tag.o"
}
export -f one; export FLAGS tag
echo $srcs | tr ' ' '\n' | xargs -P "${JOBS:-8}" -I{} bash -c 'one {}'
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 $objs -o variants/libhip_raytracer_$tag.so
rm -f $objs
echo built $tag
