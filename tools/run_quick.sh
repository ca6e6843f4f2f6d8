# usage: bash tools/run_quick.sh OUT_DIR : gpu tests (stop at first failure), then kernel trace of the C3 bench
OUT=${1:?usage: bash tools/run_quick.sh OUT_DIR}
mkdir -p "$OUT"
(time python -m pytest tests -m gpu -x -q 2>&1 | tail -30) > "$OUT/tests.log" 2>&1
grep -n "passed\|failed" "$OUT/tests.log"
python bench.py --full --no-cpu-baseline --no-c4 2> "$OUT/bench.err" | python -c "
import sys, json
for l in sys.stdin:
    if l.startswith('{'):
        d = json.loads(l); print(d['value'], d['stage_ms'], d['cold_solve']['per_call_ms'], d['config']['pcg_iters_per_call'])
"
bash tools/ktrace.sh "$OUT" > /dev/null 2>&1
OUT="$OUT" python - <<'PY'
import csv, os
rows=list(csv.DictReader(open(os.path.join(os.environ['OUT'], 'kernel_stats.csv'))))
for r in rows[:22]:
    print('%-40s calls %5s avg %9.1f us  %5s%%' % (r['Name'].split('(')[0][:40], r['Calls'], float(r['AverageNs'])/1e3, r['Percentage']))
PY
