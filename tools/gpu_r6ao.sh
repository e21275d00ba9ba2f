# final tree re-check (rebuilt library): whole GPU suite incl. full-size oracle tests, smoke, a default bench line
O=${OUT_DIR:-out}/r6ao
mkdir -p $O
timeout -k 10 900 python -u -m pytest -x -q --timeout 300 --timeout-method thread tests -m gpu \
  --ignore=tests/test_gpu_fullsize_oracle.py > $O/tests1.log 2>&1 || exit 1
timeout -k 10 400 python -u -m pytest -x -q --timeout 300 --timeout-method thread tests/test_gpu_fullsize_oracle.py \
  -m gpu > $O/tests2.log 2>&1 || exit 1
timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 || exit 1
timeout -k 10 400 python -u bench.py --full > $O/bench.json 2> $O/bench.err || exit 1
