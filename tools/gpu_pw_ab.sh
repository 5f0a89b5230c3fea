#!/bin/bash
# A/B of the cls FT step (point-wise kernels): the tree library against
# build/abx/lib*.so, after the T-Net / data GPU tests on the tree library;
# alternated 3x on one box.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
out=${PCADV_OUT:-bench_out}  # where the logs go
mkdir -p "$out"
tree=adversarial_learning_on_pointclouds_amd/lib/libpcadv.so
timeout -k 10 300 python -u -m pytest -x -q --timeout 120 --timeout-method thread -m gpu tests/test_gpu_tnet.py tests/test_gpu_data.py -k "not seg" > "$out"/pw_tests.log 2>&1 || { tail -20 "$out"/pw_tests.log; exit 1; }
tail -1 "$out"/pw_tests.log
for i in 1 2 3; do
  for lib in build/abx/lib*.so $tree; do
    PCADV_LIB=$lib timeout -k 10 200 python bench.py --repeats 3 --config cls_ft --steps 200 --warmup 20 --no-cpu > "$out"/pw_ab.json 2>/dev/null || { echo "bench failed"; exit 1; }
    python -c "import json,sys; d=json.loads(open(sys.argv[2]).read().strip().splitlines()[-1]); print('AB', sys.argv[1], d['ms_per_step'])" $(basename $lib) "$out"/pw_ab.json
  done
done
