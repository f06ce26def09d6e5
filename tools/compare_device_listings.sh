#!/bin/bash
# Proves that a change left the device code alone: builds the gfx950 device listing of every kernel-holding compilation of the
# library from two source trees and compares each pair byte for byte, after replacing the per-file hash the compiler embeds
# (__hip_cuid_<hex>) by a constant.  No GPU needed.  Which compilations those are, and with which flags, is the table of NEW_TREE's
# gym-mapf_amd/csrc/Makefile: its `listings` rules compile both trees (SRCDIR names the tree), so OLD_TREE needs no such target.
#
#   tools/compare_device_listings.sh OLD_TREE NEW_TREE WORK_DIR [JOBS]     (trees: repository roots; exit 0 = all identical)
#
# A unit whose bytes differ is compared again kernel by kernel (tools/compare_kernels.py): a change that renames or merges kernels
# moves symbols, function numbers and the kernels' order, and still leaves every instance its code, descriptor and metadata
# entry.  Such a unit is reported as "same code" with its count of paired kernels; anything else as DIFFERENT, pair by pair.
# Translation units of NEW_TREE that are not in the table must hold no kernel: their listings are checked for an empty
# kernel list as well.  A unit of the table that OLD_TREE does not have yet is compiled from NEW_TREE alone and reported as new.
set -u
OLD=$(cd "$1" && pwd); NEW=$(cd "$2" && pwd); mkdir -p "$3"; WORK=$(cd "$3" && pwd); JOBS=${4:-8}
MK="$NEW/gym-mapf_amd/csrc/Makefile"
UNITS=$(make -s --no-print-directory -f "$MK" print-kernel-units print-added-kernel-units 2>/dev/null || make -s --no-print-directory -f "$MK" print-kernel-units)   # name, source unit: both tables
HOST=$(for f in "$NEW"/gym-mapf_amd/csrc/*.hip; do unit=$(basename "$f" .hip); echo "$UNITS" | grep -q " $unit\$" || echo "$unit"; done)

build() {   # side, tree, names: the listings into $WORK/side/raw, their masked copies into $WORK/side
    local side=$1 tree=$2 name; shift 2
    make -k -j"$JOBS" -f "$MK" SRCDIR="$tree/gym-mapf_amd/csrc" LISTDIR="$WORK/$side/raw" $(printf "$WORK/$side/raw/%s.s " "$@") \
        > "$WORK/$side.make.log" 2>&1 || echo "FAILED to compile some of $side: see $WORK/$side.make.log"
    for name in "$@"; do
        rm -f "$WORK/$side/$name.s"
        [ -f "$WORK/$side/raw/$name.s" ] && sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$WORK/$side/raw/$name.s" > "$WORK/$side/$name.s"
    done
}
build old "$OLD" $(echo "$UNITS" | while read -r name unit; do [ -f "$OLD/gym-mapf_amd/csrc/$unit.hip" ] && echo "$name"; done)
build new "$NEW" $(echo "$UNITS" | cut -d' ' -f1) $HOST

status=0
echo "device listings, hipcc -S --cuda-device-only, __hip_cuid_* masked: old tree vs new tree (identical: byte for byte; same code: kernel by kernel)"
while read -r name unit; do
    if [ ! -f "$OLD/gym-mapf_amd/csrc/$unit.hip" ] && [ -s "$WORK/new/$name.s" ]; then
        echo "new unit   $name.s  $(wc -l < "$WORK/new/$name.s") lines  $(grep -c '^  - .agpr_count:' "$WORK/new/$name.s") kernels"
    elif cmp -s "$WORK/old/$name.s" "$WORK/new/$name.s" && [ -s "$WORK/new/$name.s" ]; then
        echo "identical  $name.s  $(wc -l < "$WORK/new/$name.s") lines  $(grep -c '^  - .agpr_count:' "$WORK/new/$name.s") kernels"
    elif [ -s "$WORK/old/$name.s" ] && [ -s "$WORK/new/$name.s" ]; then
        python3 "$NEW/tools/compare_kernels.py" "$WORK/old/$name.s" "$WORK/new/$name.s" "$name.s" || status=1
    else
        echo "DIFFERENT  $name.s"; status=1
    fi
done <<< "$UNITS"
for unit in $HOST; do
    n=$(grep -c '^  - .agpr_count:' "$WORK/new/$unit.s")
    if [ -f "$WORK/new/$unit.s" ] && [ "$n" = 0 ]; then echo "no kernel  $unit.s"; else echo "HAS KERNELS ($n)  $unit.s"; status=1; fi
done
exit $status
