#!/bin/bash
# `apd --images-on host` against `--images-on gpu` on the ten-view 6208x4128 folder of tools/e2e_timing.sh: RUNS runs each,
# alternating, with DVP_HOST_TIMING=1 and without the fusion (it reads no level image); tools/images_summary.py folds the logs.
# GPU box, repo root.
# usage: tools/images_timing.sh [OUT=/tmp/images_timing] [RUNS=3] [W=6208] [H=4128] [VIEWS=10] [SRC=9]
set -e -o pipefail
OUT=${1:-/tmp/images_timing}; RUNS=${2:-3}; W=${3:-6208}; H=${4:-4128}; NV=${5:-10}; NS=${6:-9}
mkdir -p "$OUT"
DS=/tmp/ds_images
rm -rf $DS
timeout -k 10 300 python tools/make_dataset.py $DS $W $H $NV $NS --jpg --torch > /dev/null
LOGS=""
for run in $(seq 1 $RUNS); do
	for mode in host gpu; do
		rm -rf $DS/APD
		( time DVP_HOST_TIMING=1 timeout -k 10 300 ./dvp-mvs_amd/apd $DS 0 --iters 3 --passes 1 --min-scale 1 --seed 3 --no-fusion --images-on $mode ) > "$OUT/${mode}_$run.log" 2>&1
		LOGS="$LOGS $OUT/${mode}_$run.log"
	done
done
python tools/images_summary.py $LOGS | tee "$OUT/summary.txt"
