#!/bin/bash
# tools/ab/build_variant.sh NAME [-DFLAG ...] : alternative build of the C ABI ($UNITS, default the contraction units gemm gemm_fp8 wgrad,
# recompiled with the flags; the product objects of every other unit reused) -> tools/ab/libNAME.so, selected at run time with SIDLSG_LIB
# (in-session A/B on one GPU box).  UNITS="wgrad" tools/ab/build_variant.sh ... recompiles one unit only.
set -e
cd "$(dirname "$0")/../../sid_lsg_amd/csrc"
. ../../tools/ab/_variant.sh
name=$1; shift
units=${UNITS:-$GEMM_UNITS}
pids=""
for u in $units; do variant_cc $name $u "$@" & pids="$pids $!"; done
for p in $pids; do wait $p; done
variant_link $name $units
