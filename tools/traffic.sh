#!/bin/bash
# HBM traffic of the bench step from PMC counters (MI355X_MICROARCH.md § HBM): two separate rocprofv3
# passes (FETCH_SIZE and WRITE_SIZE do not fit one pass), counters only, then tools/traffic.py
# writes profiles/traffic_<mode>_<prec>_b<B>.json. usage: bash tools/traffic.sh <tag> [mode]
set -o pipefail
TAG=${1:-traffic}
MODE=${2:-train}
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${VCG_OUT:-bench_out}  # where logs and result lines go
mkdir -p "$OUT"
export TMPDIR=/tmp
for C in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 900 rocprofv3 --pmc $C --output-format csv -d $OUT/${TAG}_$C -o run -- python bench.py --full --mode $MODE --steps 1 --warmup 1 --no-cpu-baseline > $OUT/${TAG}_$C.log 2>&1 || { echo "pmc $C failed"; tail -20 $OUT/${TAG}_$C.log; exit 1; }
done
python tools/traffic.py $OUT/${TAG}_FETCH_SIZE $OUT/${TAG}_WRITE_SIZE 3 $MODE
