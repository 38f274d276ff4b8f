#!/bin/bash
# Do two source trees compile to the same device code? (dev tool, no GPU needed)
# Compiles, device-only to assembly, every .hip unit of both trees -- the sixteen TERRA_TU units of render_kernels.hip (0 - 3 camera, 4 - 7 ray-sourced, 8 - 11 lens, 12 - 15 point), unit_kernels.hip,
# tree_build_device.hip, aov_kernels.hip with its ray-sourced, lens and point units (TERRA_TU 4, 8, 12), denoise_kernels.hip, variance_kernels.hip, temporal_kernels.hip, query_kernels.hip, bake_kernels.hip, probe_kernels.hip, nearest_kernels.hip and multi_hit_kernels.hip -- with exactly the FLAGS of this tree's
# terra_amd/build.py (plus any extra -D given), strips what is not code -- comment lines, .file/.ident, and the lines naming the per-compilation
# __hip_cuid_<hash> symbol, trailing comments and the number a function's labels carry for its place in the unit (.LBB<n>_, .Lfunc_end<n>: a function keeps
# its body when another one leaves the unit) -- and reports per unit "identical" or the symbols whose bodies differ. A unit that only one tree has is reported as such and
# counts as a difference.
# usage: tools/isa_same.sh <tree A> <tree B> <scratch dir> [extra -D flags]
#   e.g. git worktree add /tmp/parent HEAD~1 && tools/isa_same.sh /tmp/parent . /tmp/isa -DTERRA_CHECK_BOUNDS=1
# A render unit takes a minute or more; at most 16 compile at a time. A unit's assembly is kept in the scratch directory under a key made of the tree's
# path, the compiler, FLAGS and the extra flags, and compiled again when a file under the tree's terra_amd/csrc or include is newer than it: a second run
# against the same parent compiles the changed tree alone, and no other tree, flag set or compiler is ever answered from it.
# Exit status: 0 all identical, 1 some unit differs, 2 a compile failed.
set -o pipefail
[ $# -ge 3 ] || { sed -n '2,13p' "$0"; exit 2; }
HERE=$(cd "$(dirname "$0")/.." && pwd)
A=$(cd "$1" && pwd) || exit 2; B=$(cd "$2" && pwd) || exit 2; mkdir -p "$3" || exit 2; S=$(cd "$3" && pwd); shift 3
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS=$(python3 -c "import runpy, sys; print(' '.join(runpy.run_path(sys.argv[1])['FLAGS']))" "$HERE/terra_amd/build.py") || exit 2
key() { printf '%s\n' "$1" "$HIPCC" "$($HIPCC --version 2>/dev/null | head -n 1)" "$FLAGS" "$2" | md5sum | cut -c1-16; }
DA=$S/$(key "$A" "$*"); DB=$S/$(key "$B" "$*")
UNITS="render_kernels.tu0 render_kernels.tu1 render_kernels.tu2 render_kernels.tu3 render_kernels.tu4 render_kernels.tu5 render_kernels.tu6 render_kernels.tu7 render_kernels.tu8 render_kernels.tu9 render_kernels.tu10 render_kernels.tu11 render_kernels.tu12 render_kernels.tu13 render_kernels.tu14 render_kernels.tu15 unit_kernels tree_build_device aov_kernels aov_kernels.tu4 aov_kernels.tu8 aov_kernels.tu12 denoise_kernels variance_kernels temporal_kernels query_kernels bake_kernels probe_kernels nearest_kernels multi_hit_kernels"
JOBS=$(nproc); [ "$JOBS" -gt 16 ] && JOBS=16
mkdir -p "$DA" "$DB"

for side in a b; do
    tree=$A; dir=$DA; [ $side = b ] && { tree=$B; dir=$DB; }
    [ $side = b ] && [ "$DA" = "$DB" ] && continue
    for u in $UNITS; do
        s=$dir/$u.s
        [ -f "$tree/terra_amd/csrc/${u%.tu*}.hip" ] || continue
        [ -s "$s" ] && [ -z "$(find "$tree/terra_amd/csrc" "$tree/include" -newer "$s" -type f -print -quit)" ] && continue
        tu=; case $u in *.tu*) tu=-DTERRA_TU=${u##*.tu};; esac
        printf '%q %s %s %s --cuda-device-only -S %q -o %q 2> %q && mv %q %q\n' "$HIPCC" "$FLAGS" "$tu" "$*" "$tree/terra_amd/csrc/${u%.tu*}.hip" "$s.tmp" "$s.err" "$s.tmp" "$s"
    done
done > "$DB/jobs.txt"
if [ -s "$DB/jobs.txt" ]; then
    echo "compiling $(wc -l < "$DB/jobs.txt") unit(s), $JOBS at a time ..." >&2
    xargs -P "$JOBS" -d '\n' -n 1 bash -c < "$DB/jobs.txt" || { echo "a compile failed; see $DA/*.err $DB/*.err" >&2; exit 2; }
fi

# code lines only, each prefixed with the symbol it belongs to (a function body, or that kernel's .amdhsa_kernel descriptor)
code_by_symbol() {
    awk '/^[ \t]*;/ || /^[ \t]*\.(file|ident)[ \t]/ || /__hip_cuid_/ { next }
         { sub(/[ \t]*;.*$/, ""); gsub(/\.LBB[0-9]+_/, ".LBB_"); gsub(/\.Lfunc_end[0-9]+/, ".Lfunc_end"); gsub(/\.Lfunc_begin[0-9]+/, ".Lfunc_begin") }
         /^[ \t]*\.type[ \t].*,@function/ { sym = $2; sub(/,@function.*/, "", sym) }
         /^[ \t]*\.amdhsa_kernel[ \t]/    { sym = $2 }
         { print (sym == "" ? "(outside any function)" : sym) "\t" $0 }
         /^[ \t]*\.size[ \t]/ || /^[ \t]*\.end_amdhsa_kernel/ { sym = "" }' "$1"
}
rc=0
for u in $UNITS; do
    [ -f "$A/terra_amd/csrc/${u%.tu*}.hip" ] || { echo "$u: only in $B"; rc=1; continue; }
    [ -f "$B/terra_amd/csrc/${u%.tu*}.hip" ] || { echo "$u: only in $A"; rc=1; continue; }
    d=$(diff <(code_by_symbol "$DA/$u.s") <(code_by_symbol "$DB/$u.s") | sed -n 's/^[<>] \([^\t]*\)\t.*/\1/p' | sort -u)
    if [ -z "$d" ]; then echo "$u: identical"; else echo "$u: DIFFERS in"; echo "$d" | sed 's/^/    /'; rc=1; fi
done
exit $rc
