# final tree: the full-size oracle tests, then the default bench (legs + cpu baseline)
O=${OUT_DIR:-out}/r6al
mkdir -p $O
timeout -k 10 800 python -u -m pytest -x -q --timeout 650 --timeout-method thread tests/test_gpu_fullsize_oracle.py -m gpu > $O/tests2.log 2>&1 || exit 1
timeout -k 10 350 python -u bench.py --full > $O/bench.txt 2> $O/bench.err || exit 1
