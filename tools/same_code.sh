#!/bin/bash
# Is the device code of this tree the device code of another checkout?  Every .hip unit of both trees is compiled to
# gfx950 assembly with build.py's flags, the __hip_cuid_* symbols (a hash of the source path) are made equal, and the
# two files are compared function by function: a plain diff, one line per unit.
#   tools/same_code.sh <parent checkout> [-DNAME[=VALUE] ...]
#   UNITS="kernels" tools/same_code.sh ../parent -DSAGE_LOOP_TIMING      # some units only (probe builds: kernels.hip)
# OUT=<dir> keeps the assembly (<dir>/parent, <dir>/here); JOBS=<n> compiles n units at a time (default 4).
# Exit status 0: every function of every unit identical.
set -u
[ $# -ge 1 ] && [ -d "$1/sage-icp_amd/csrc" ] || { echo "usage: $0 <parent checkout> [-D...]" >&2; exit 2; }
parent=$(cd "$1" && pwd); shift
here=$(cd "$(dirname "$0")/.." && pwd)
hipcc=${HIPCC:-/opt/rocm/bin/hipcc}
out=${OUT:-$(mktemp -d)}
flags=$(python3 -c "import sys; sys.path.insert(0, '$here/sage-icp_amd'); import build; print(' '.join(build.FLAGS))") || exit 2
units=${UNITS:-$(cd "$here/sage-icp_amd/csrc" && ls *.hip | sed 's/\.hip$//')}
mkdir -p "$out/parent" "$out/here"

for u in $units; do
    for side in parent here; do
        [ $side = parent ] && root=$parent || root=$here
        echo "$hipcc $flags $* --cuda-device-only -S $root/sage-icp_amd/csrc/$u.hip -o $out/$side/$u.s 2> $out/$side/$u.err"
    done
done | xargs -P "${JOBS:-4}" -I{} sh -c '{}' || { echo "a unit did not compile: see $out/*/*.err" >&2; exit 2; }

# one file per function: from its .type line to its .size line
split() {
    sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_/g' "$1" |
        awk -v dir="$2" '/^\t\.type\t.*,@function/ { split($2, a, ","); f = dir "/" (++n) "." substr(a[1], 1, 200); names[n] = a[1] }
                         f { print > f }
                         f && /^\t\.size\t/ { close(f); f = "" }'
}

echo "$hipcc $flags $* --cuda-device-only -S <unit>.hip at the parent and here, compared function by function (__hip_cuid_* symbols made equal):"
total=0; same=0; status=0
for u in $units; do
    rm -rf "$out/fn" && mkdir -p "$out/fn/parent" "$out/fn/here"
    split "$out/parent/$u.s" "$out/fn/parent"
    split "$out/here/$u.s" "$out/fn/here"
    n=$(ls "$out/fn/here" | wc -l)
    differing=$(diff -rq "$out/fn/parent" "$out/fn/here" | wc -l)
    whole="whole file DIFFERS"
    if diff -q <(sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_/g' "$out/parent/$u.s") \
               <(sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_/g' "$out/here/$u.s") > /dev/null; then
        whole="whole file identical but for __hip_cuid_*"
    else
        status=1
    fi
    printf "%-22s functions %4d  differing %d  %s\n" "$u.s" "$n" "$differing" "$whole"
    [ "$differing" -gt 0 ] && diff -rq "$out/fn/parent" "$out/fn/here" | sed 's/^/    /' | c++filt | cut -c1-220
    total=$((total + n)); same=$((same + n - differing))
done
rm -rf "$out/fn"
echo "total: $total functions, $same identical"
[ "$same" -eq "$total" ] && exit $status || exit 1
