#!/bin/bash
# tools/ab/build_skip_variant.sh : measurement build of the C ABI with -DSIDLSG_EXP_SKIP (common.h): kernels of the families named by
# $SIDLSG_EXP_SKIP_FAMILIES (bit mask over SIDLSG_FAM_*) are not launched.  WRONG results by construction; the step-time difference against the
# same library with mask 0 is what that family costs the iteration (its exposed time, contention included) -> tools/family_exposed_cost.sh
set -e
cd "$(dirname "$0")/../../sid_lsg_amd/csrc"
. ../../tools/ab/_variant.sh
units="$GEMM_UNITS norm attention"      # the units whose launches belong to a traced family
pids=""
for u in $units; do variant_cc skip $u -DSIDLSG_EXP_SKIP & pids="$pids $!"; done
for p in $pids; do wait $p; done
variant_link skip $units
