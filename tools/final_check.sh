#!/bin/bash
# Last check of the final tree: full GPU suite + smoke -> $OUT/final/,
# then two cfg4 lines -> $OUT/cfg4h/   (OUT: an output folder, default ./out)
set -u
cd "$(dirname "$0")/.."
OUT=${OUT:-out}
mkdir -p "$OUT/final" "$OUT/cfg4h"
timeout -k 10 700 python -u -m pytest tests -m gpu -q -rf --durations=10 --timeout 300 --timeout-method thread \
  > "$OUT/final/pytest_gpu.log" 2>&1; rc=$?; tail -1 "$OUT/final/pytest_gpu.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/final/smoke.log" 2>&1; rc=$?
tail -1 "$OUT/final/smoke.log"; [ $rc -eq 0 ] || exit $rc
for i in 1 2; do
  timeout -k 10 600 python bench.py --full --workload cfg4 --steps 2 --warmup 1 --no-cpu-baseline > "$OUT/cfg4h/q_$i.json" 2> "$OUT/cfg4h/q_$i.err" || { echo "cfg4 rc=$?"; exit 3; }
  python3 -c "import json;d=json.load(open('$OUT/cfg4h/q_$i.json'));print('cfg4', d['value'], d['ms_per_step'], d['roofline']['frac'], d.get('verified','')[:6])"
done
