#!/bin/bash
# A second build of the HIP library for A/B timing against the in-tree one (MU_LIB_PATH): tools/build_variant.sh NAME [SOURCE_DIR]
# -> gpurun_variants/libmu_NAME.so (used by tools/ab_bench.py).  Debug aid, not part of the product build.
# SOURCE_DIR: a checkout of this repository (default: this tree), e.g. `git worktree add ../parent HEAD~1`.  The library is built by
# that checkout's own maskunet_amd/csrc/Makefile -- its file list and flags -- with the objects and the library redirected here.
# (A checkout whose Makefile has no OBJDIR yet leaves its objects in its own csrc/; the library still lands here.)
set -e
NAME=${1:?usage: tools/build_variant.sh NAME [SOURCE_DIR]}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=$(cd "${2:-$ROOT}" && pwd)
OUT=$ROOT/gpurun_variants
mkdir -p "$OUT"
make -C "$SRC/maskunet_amd/csrc" -j8 OBJDIR="$OUT/obj_$NAME" LIB="$OUT/libmu_$NAME.so"
rm -rf "$OUT/obj_$NAME"
echo built "$OUT/libmu_$NAME.so"
