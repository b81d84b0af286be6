#!/bin/bash
# Per-view wall time of the FIRST_INIT plane prior through `apd`, host path and device path (profiles/prior_timing.txt):
# three-view folders at 1552x1032 (make_dataset.py's own point count) and 6208x4128 (10 000 points per view), one run per mode,
# DVP_HOST_TIMING=1 lap lines of InuputInitialization / CudaSpaceInitialization.  Needs a GPU (the folders are rendered with --torch).
# usage: tools/prior_timing.sh [OUT_FILE]
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-/dev/stdout}
T=$(mktemp -d)
lscpu | grep -E "Model name|^CPU\(s\)" >> "$OUT"
for size in "1552 1032 0" "6208 4128 10000"; do
  set -- $size
  W=$1; H=$2; N=$3
  echo "==== $W x $H" >> "$OUT"
  timeout -k 10 300 python3 tools/make_dataset.py $T/base_$W $W $H 3 2 --prior --torch > /dev/null || exit $?
  if [ "$N" != "0" ]; then python3 tools/thin_sfm.py $T/base_$W $N >> "$OUT" || exit $?; else wc -l $T/base_$W/sfm/*.txt >> "$OUT"; fi
  for mode in host gpu; do
    cp -r $T/base_$W $T/${mode}_$W || exit $?
    echo "---- --prior-on $mode" >> "$OUT"
    DVP_HOST_TIMING=1 timeout -k 10 240 dvp-mvs_amd/apd $T/${mode}_$W 0 --iters 1 --passes 0 --no-fusion --seed 9 --prior-on $mode > $T/log_${mode}_$W.txt 2>&1 || exit $?
    grep -E "plane prior|Plane prior|No dep" $T/log_${mode}_$W.txt >> "$OUT"
  done
  for v in 0 1 2; do cmp $T/host_$W/APD/0000000$v/depths.dmb $T/gpu_$W/APD/0000000$v/depths.dmb && echo "view $v: depths.dmb identical" >> "$OUT"; done
done
rm -rf "$T"
