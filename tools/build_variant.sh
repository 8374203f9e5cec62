#!/bin/bash
# Build a libsr variant: tools/build_variant.sh NAME [extra hipcc flags...]
# -> schwarzschild-raytracer_amd/lib/variants/libsr_NAME.so (A/B timing only).
# KERNEL=path overrides the geodesic kernel source (e.g. a file made with
# `git show REV:schwarzschild-raytracer_amd/csrc/kernels/geodesic.hip`; it
# must match this tree's device_scene.h). WAVES: the small instantiation's
# waves per SIMD (default: the Makefile's). The files and the flags are the
# Makefile's (its `variant` target).
set -e
PKG=$(cd "$(dirname "$0")/.." && pwd)/schwarzschild-raytracer_amd
NAME=$1; shift
[ -z "$KERNEL" ] || export KERNEL=$(realpath "$KERNEL")
make -s -C "$PKG" -j10 variant NAME="$NAME" EXTRA="$*"
echo "$NAME: $(grep -E '^\s+\.(vgpr_count|sgpr_count|vgpr_spill_count)' "$PKG/build/variants/$NAME/geodesic.s" | head -3 | tr -s ' ' | tr '\n' ' ')"
