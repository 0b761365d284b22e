# A/B of the pair-packed stem (default) against the C = 8 stem (VCG_NO_STEM_PAIR=1), after its tests.
set -o pipefail
cd "$GRAFT_REPO_ROOT"
OUT=${VCG_OUT:-bench_out}  # where logs and result lines go
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest tests/test_gpu_kernels.py -q -m gpu -x --timeout 300 --timeout-method thread -k "stem_pair or window_frames or conv_fwd or conv_wgrad" > $OUT/stem_tests.log 2>&1 || { echo "kernel tests failed"; tail -30 $OUT/stem_tests.log; exit 1; }
tail -1 $OUT/stem_tests.log
timeout -k 10 900 python -u -m pytest tests/test_gpu_parity.py tests/test_gpu_long_video.py -q -m gpu -x --timeout 300 --timeout-method thread > $OUT/stem_parity.log 2>&1 || { echo "parity tests failed"; tail -30 $OUT/stem_parity.log; exit 1; }
tail -1 $OUT/stem_parity.log
for i in 1 2; do
  VCG_NO_STEM_PAIR=1 timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > $OUT/stem_a$i.log 2>&1 || exit 2
  python -c "import json;d=json.loads(open('$OUT/stem_a$i.log').read().strip().splitlines()[-1]);print('c8',d['value'],d['ms_per_step'])"
  timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > $OUT/stem_c$i.log 2>&1 || exit 2
  python -c "import json;d=json.loads(open('$OUT/stem_c$i.log').read().strip().splitlines()[-1]);print('pair',d['value'],d['ms_per_step'])"
done
