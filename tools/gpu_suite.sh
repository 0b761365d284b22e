#!/bin/bash
# The whole -m gpu suite, smoke() and one bench line at HEAD (the driver's round-end checks, rehearsed).
set -o pipefail
OUT=${VCG_OUT:-bench_out}  # where logs and result lines go
mkdir -p "$OUT"
TAG=${1:-suite}
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -q -rf --timeout 300 --timeout-method thread > $OUT/${TAG}_tests.log 2>&1 || { echo "tests failed"; grep -E "^E |FAILED" $OUT/${TAG}_tests.log | head -20; tail -5 $OUT/${TAG}_tests.log; exit 7; }
tail -2 $OUT/${TAG}_tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 || { echo "smoke failed"; tail -20 $OUT/${TAG}_smoke.log; exit 8; }
tail -2 $OUT/${TAG}_smoke.log
timeout -k 10 400 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { echo "bench failed"; tail -20 $OUT/${TAG}_bench.err; exit 9; }
python -c "import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print('bench', d['value'], d['ms_per_step'], d['roofline']['frac'])" $OUT/${TAG}_bench.json
