# merged rollout launch (final form): bit-identity + parity subset, then the default bench twice
O=${OUT_DIR:-out}/r6aa
mkdir -p $O
timeout -k 10 600 python -u -m pytest -x -q --timeout 300 --timeout-method thread tests/test_gpu_byte_targets.py \
  tests/test_gpu_parity.py tests/test_gpu_fullsize.py -m gpu > $O/tests.log 2>&1 || exit 1
for r in 1 2; do
  timeout -k 10 600 python -u bench.py --full --cpu_baseline 0 > $O/bench_$r.txt 2>&1 || exit 1
done
