#!/bin/bash
# tools/ab/build_combo.sh NAME "ATTN_FLAGS" "GEMM_FLAGS" : alternative build of the C ABI with attention.hip and / or the contraction
# units (gemm gemm_fp8 wgrad) recompiled with the given -D flags (empty string = reuse the product objects) -> tools/ab/libNAME.so,
# selected at run time with SIDLSG_LIB (in-session A/B on one GPU box).
set -e
cd "$(dirname "$0")/../../sid_lsg_amd/csrc"
. ../../tools/ab/_variant.sh
name=$1; aflags=$2; gflags=$3
units=""; pids=""
if [ -n "$aflags" ]; then units="attention"; variant_cc $name attention $aflags & pids="$pids $!"; fi
if [ -n "$gflags" ]; then
    units="$units $GEMM_UNITS"
    for u in $GEMM_UNITS; do variant_cc $name $u $gflags & pids="$pids $!"; done
fi
for p in $pids; do wait $p; done
variant_link $name $units
