# Sourced by the build_*.sh scripts of this directory (cwd: sid_lsg_amd/csrc).  The compile flags, the per-file extras and the list of
# units all come from build.py, so a variant library always holds every object of the product library.
GEMM_UNITS="gemm gemm_fp8 wgrad"      # the contraction units: what a -D switch of gemm_core.h / gemm_p8.h can reach
bp() { python3 -c "import build; $1"; }
variant_cc() {      # NAME UNIT [FLAG ...] -> build/UNIT_NAME.o
    local name=$1 unit=$2; shift 2
    /opt/rocm/bin/hipcc $(bp "print(' '.join(build.FLAGS + build.EXTRA.get('$unit.hip', [])))") "$@" -c $unit.hip -o build/${unit}_$name.o
}
variant_link() {    # NAME UNIT ... -> tools/ab/libNAME.so: the named units' variant objects, the product objects of every other unit
    local name=$1 objs="" u; shift
    for u in $(bp "print(' '.join(s[:-4] for s in build.SOURCES))"); do
        case " $* " in *" $u "*) objs="$objs build/${u}_$name.o" ;; *) objs="$objs build/$u.o" ;; esac
    done
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs -o ../../tools/ab/lib$name.so
    echo tools/ab/lib$name.so
}
