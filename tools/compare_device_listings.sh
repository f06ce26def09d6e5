#!/bin/bash
# Proves that a change left the device code alone: compiles the gfx950 device listing (hipcc -S --cuda-device-only, the
# Makefile's flags) of every kernel-holding compilation of the library from two source trees and compares each pair byte
# for byte, after replacing the per-file hash the compiler embeds (__hip_cuid_<hex>) by a constant.  No GPU needed.
#
#   tools/compare_device_listings.sh OLD_TREE NEW_TREE WORK_DIR [JOBS]     (trees: repository roots; exit 0 = all identical)
#
# Translation units of NEW_TREE that are not in the list must hold no kernel: their listings are checked for an empty
# kernel list as well.  A unit of the list that OLD_TREE does not have yet is compiled from NEW_TREE alone and reported as new.
set -u
OLD=$(cd "$1" && pwd); NEW=$(cd "$2" && pwd); WORK=$3; JOBS=${4:-8}
mkdir -p "$WORK/old" "$WORK/new"

# name | unit | extra flags
UNITS="mapf_lg_kernels|mapf_lg_kernels|
mapf_lg_rollout|mapf_lg_rollout|
mapf_lg_limit|mapf_lg_limit|
mapf_lg_budget|mapf_lg_budget|
mapf_transitions|mapf_transitions|
mapf_lq_step|mapf_lq_step|-mllvm -amdgpu-kernarg-preload-count=14"
for k in 8 4 2; do for r in 1 0; do UNITS="$UNITS
mapf_lq_rollout_k${k}_r${r}|mapf_lq_rollout|-DMAPF_LQ_K=$k -DMAPF_LQ_RECORD=$r"; done; done
for k in 4 2; do for r in 1 0; do UNITS="$UNITS
mapf_lq_limit_k${k}_r${r}|mapf_lq_limit|-DMAPF_LQ_K=$k -DMAPF_LQ_RECORD=$r"; done; done
for g in 0 1 2 3; do UNITS="$UNITS
mapf_kernels_g$g|mapf_kernels|-DMAPF_GROUP=$g"; done

listing() {   # tree, side, name, unit, flags
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -I"$1/include" -Wall $5 -S --cuda-device-only \
        "$1/gym-mapf_amd/csrc/$4.hip" -o "$WORK/$2/$3.raw.s" 2>/dev/null &&
        sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$WORK/$2/$3.raw.s" > "$WORK/$2/$3.s" && rm "$WORK/$2/$3.raw.s"
}
export -f listing; export WORK
{
    echo "$UNITS" | while IFS='|' read -r name unit flags; do
        [ -s "$WORK/old/$name.s" ] || [ ! -f "$OLD/gym-mapf_amd/csrc/$unit.hip" ] || printf '%s\0%s\0%s\0%s\0%s\0' "$OLD" old "$name" "$unit" "$flags"
        printf '%s\0%s\0%s\0%s\0%s\0' "$NEW" new "$name" "$unit" "$flags"
    done
    for f in "$NEW"/gym-mapf_amd/csrc/*.hip; do
        unit=$(basename "$f" .hip)
        echo "$UNITS" | grep -q "|$unit|" || printf '%s\0%s\0%s\0%s\0%s\0' "$NEW" new "$unit" "$unit" ""
    done
} | xargs -0 -n 5 -P "$JOBS" bash -c 'listing "$@" || echo "FAILED to compile $2/$3"' _

status=0
echo "device listings, hipcc -S --cuda-device-only, __hip_cuid_* masked: old tree vs new tree"
while IFS='|' read -r name unit flags; do
    if [ ! -f "$OLD/gym-mapf_amd/csrc/$unit.hip" ] && [ -s "$WORK/new/$name.s" ]; then
        echo "new unit   $name.s  $(wc -l < "$WORK/new/$name.s") lines  $(grep -c '^  - .agpr_count:' "$WORK/new/$name.s") kernels"
    elif cmp -s "$WORK/old/$name.s" "$WORK/new/$name.s" && [ -s "$WORK/new/$name.s" ]; then
        echo "identical  $name.s  $(wc -l < "$WORK/new/$name.s") lines  $(grep -c '^  - .agpr_count:' "$WORK/new/$name.s") kernels"
    else
        echo "DIFFERENT  $name.s"; status=1
    fi
done <<< "$UNITS"
for f in "$NEW"/gym-mapf_amd/csrc/*.hip; do
    unit=$(basename "$f" .hip)
    echo "$UNITS" | grep -q "|$unit|" && continue
    n=$(grep -c '^  - .agpr_count:' "$WORK/new/$unit.s")
    if [ -f "$WORK/new/$unit.s" ] && [ "$n" = 0 ]; then echo "no kernel  $unit.s"; else echo "HAS KERNELS ($n)  $unit.s"; status=1; fi
done
exit $status
