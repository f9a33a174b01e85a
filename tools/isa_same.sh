#!/bin/bash
# Do the device functions of <old.hip> come out instruction for instruction from <new.hip> [<new2.hip> ...] together?
# usage: tools/isa_same.sh <old.hip> <new.hip> [<new2.hip> ...] [-- extra hipcc flags, e.g. -DMRG_EXPERIMENT]
# (<old.hip> may lie anywhere, e.g. `git show HEAD~1:mrgingham_amd/csrc/cc.hip > /tmp/cc_old.hip`: csrc/ is on the include path)
# Every file is compiled with the library's flags to device assembly; of every function `_ZN3mrg...:` (and of the kernels
# of an anonymous namespace, `_ZN12_GLOBAL__N_1...:`; functions only, not the constant tables) the text up to its
# .Lfunc_end is kept, without comments (`;` to the end of the line), with every local label `.L<name><number>` written `.L`
# (their numbering differs between any two compilations), without trailing blanks and empty lines.  One line per function:
# `same` or `DIFFERENT`; `MISSING` / `EXTRA` for a symbol only one side has.  Exit status 1 unless all are `same`.
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OLD=$1; shift
NEW=()
while [ $# -gt 0 ] && [ "$1" != -- ]; do NEW+=("$1"); shift; done
[ "${1:-}" = -- ] && shift
[ -n "$OLD" ] && [ ${#NEW[@]} -gt 0 ] || { sed -n '2,3p' "$0"; exit 2; }
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
functions_of() {  # <file.hip> <directory>: one file per function, named by its symbol
    mkdir -p "$2"
    /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=off -I"$R/mrgingham_amd/csrc" "${@:3}" \
        --offload-device-only -S "$1" -o "$2.s"
    awk -v d="$2" '
        /^[ \t]*\.type[ \t].*,@function/ { f = $2; sub(/,.*/, "", f); isfn[f] = 1 }
        /^_ZN(3mrg|12_GLOBAL__N_1)[A-Za-z0-9_]*:/ { n = substr($1, 1, length($1) - 1); out = (n in isfn) ? d "/" n : "" }
        /^\.Lfunc_end/           { out = "" }
        out != "" { l = $0; sub(/;.*/, "", l); gsub(/\.L[A-Za-z_]*[0-9_]*/, ".L", l); sub(/[ \t]+$/, "", l); if (l != "") print l > out }' "$2.s"
}
functions_of "$OLD" "$T/old" "$@"
for f in "${NEW[@]}"; do functions_of "$f" "$T/new" "$@"; done
bad=0
for s in $(ls "$T/old" "$T/new" | grep -E '^_ZN(3mrg|12_GLOBAL__N_1)' | sort -u); do
    if [ ! -e "$T/new/$s" ]; then r=MISSING; elif [ ! -e "$T/old/$s" ]; then r=EXTRA
    elif cmp -s "$T/old/$s" "$T/new/$s"; then r=same; else r=DIFFERENT; fi
    [ $r = same ] || bad=1
    echo "$r $(wc -l < "$T/$([ $r = EXTRA ] && echo new || echo old)/$s") lines $(echo "$s" | c++filt | cut -c1-150)"
done
exit $bad
