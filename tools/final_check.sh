# the whole check of a finished change, on a machine with the GPU: gpu tests, smoke, the benchmark with every leg (--full)
# usage: bash tools/final_check.sh OUT_DIR
OUT=${1:?usage: bash tools/final_check.sh OUT_DIR}
mkdir -p "$OUT"
(time python -m pytest tests -x -q -m gpu 2>&1 | tail -14) > "$OUT/tests.log" 2>&1
grep -n "passed\|failed" "$OUT/tests.log"
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | grep -v amdgpu.ids | tail -2
(time python bench.py --full) > "$OUT/bench.json" 2> "$OUT/bench.err"
tail -3 "$OUT/bench.err"
OUT="$OUT" python - <<'PY'
import json, os
d = json.loads([l for l in open(os.path.join(os.environ['OUT'], 'bench.json')) if l.startswith('{')][-1])
print(d['value'], d['stage_ms'], d['roofline']['frac'], d['roofline']['traffic_stale'], d['c4_single_gpu_ms'], d['c4_single_gpu']['stage_ms'], d['cpu_baseline']['value'], d['cpu_baseline']['spsolve_full_s'])
PY
