#!/bin/bash
# usage (on the GPU box, from the repo root): bash tools/gpu_check.sh <tag> [soak seconds] — GPU test suite, soak, bench on both workloads;
# everything goes to $OUT_DIR/<tag>_* (default: out/); prints a short summary.  Steps are chained: a failing step stops the run.
tag=$1; soak=${2:-60}; out=${OUT_DIR:-out}; mkdir -p $out
python -m pytest tests -m gpu -x -q > $out/${tag}_tests.log 2>&1; rc=$?
tail -3 $out/${tag}_tests.log
[ $rc -ne 0 ] && { grep -E "^E|Error|FAILED" $out/${tag}_tests.log | head -20; exit 1; }
if [ "$soak" != "0" ]; then
  timeout -k 10 $((soak + 120)) python tools/soak.py $soak $RANDOM > $out/${tag}_soak.log 2>&1; rc=$?
  tail -1 $out/${tag}_soak.log
  [ $rc -ne 0 ] && { grep MISMATCH $out/${tag}_soak.log; exit 1; }
fi
python bench.py --full --no-cpu-baseline > $out/${tag}_bench.json 2> $out/${tag}_bench.err || { tail -5 $out/${tag}_bench.err; exit 1; }
python bench.py --full --workload pairs --no-cpu-baseline > $out/${tag}_bench_pairs.json 2> $out/${tag}_bench_pairs.err || { tail -5 $out/${tag}_bench_pairs.err; exit 1; }
python bench.py --full --no-labels --no-cpu-baseline > $out/${tag}_bench_nolabels.json 2> $out/${tag}_bench_nolabels.err || { tail -5 $out/${tag}_bench_nolabels.err; exit 1; }
python tools/bench_summary.py $out/${tag}_bench.json $out/${tag}_bench_pairs.json $out/${tag}_bench_nolabels.json
