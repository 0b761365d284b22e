#!/bin/bash
# End-of-round measurement on one box: the train bench line (with its CPU baseline), PMC traffic + MFMA busy of the
# train step, and the scoring lines for both BN semantics (tools/gpu_measure.sh). usage: bash tools/final_measure.sh <tag>
set -o pipefail
TAG=${1:-fin}
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${VCG_OUT:-bench_out}  # where logs and result lines go
mkdir -p "$OUT"
timeout -k 10 600 python bench.py --full > $OUT/${TAG}_train.json 2> $OUT/${TAG}_train.err || { echo "bench failed"; tail -20 $OUT/${TAG}_train.err; exit 1; }
tail -1 $OUT/${TAG}_train.json | cut -c1-300
bash tools/traffic.sh ${TAG}_tr > $OUT/${TAG}_tr.txt 2>&1 || { echo "traffic failed"; exit 2; }
bash tools/mfma.sh ${TAG}_mf > $OUT/${TAG}_mf.txt 2>&1 || { echo "mfma failed"; exit 3; }
bash tools/gpu_measure.sh ${TAG}_m
