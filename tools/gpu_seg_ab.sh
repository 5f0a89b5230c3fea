#!/bin/bash
# Seg A/B: GPU seg tests on the tree's library, then the seg bench alternated
# between build/ab/libA.so (A) and the tree's libpcadv.so (B), then a kernel
# trace of B.  Every GPU step has its own time limit; the first failure ends it.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
out=${PCADV_OUT:-bench_out}  # where the logs go
mkdir -p "$out"
timeout -k 10 400 python -u -m pytest tests/test_gpu_seg.py -x -q --timeout 120 --timeout-method thread > "$out"/sab_pytest.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -1 "$out"/sab_pytest.log
[ $rc -eq 0 ] || exit $rc
for i in 1 2 3; do
  for v in A B; do
    if [ $v = A ]; then lib=build/ab/libA.so; else lib=adversarial_learning_on_pointclouds_amd/lib/libpcadv.so; fi
    PCADV_LIB=$lib timeout -k 10 200 python bench.py --full --config seg --steps 20 --warmup 3 --no-cpu > "$out"/sab_$v$i.log 2>&1
    rc=$?; [ $rc -eq 0 ] || { echo "bench $v rc=$rc"; exit $rc; }
    python -c "import json,sys; d=json.loads([l for l in open(sys.argv[1]) if '\"metric\"' in l][-1]); print('$v', d['ms_per_step'], d['roofline']['avg_launch_us'])" "$out"/sab_$v$i.log
  done
done
rm -rf "$out"/sab_trace
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$out"/sab_trace -o run --output-format csv -- python bench.py --config seg --no-cpu --steps 5 --warmup 1 > "$out"/sab_trace.log 2>&1 || exit 1
python tools/kstats.py "$out"/sab_trace/run_kernel_trace.csv > "$out"/sab_kstats.txt; head -12 "$out"/sab_kstats.txt
