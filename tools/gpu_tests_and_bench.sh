set -x
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}
mkdir -p "$OUT"
cd "$R"
timeout -k 10 800 python -m pytest tests -x -q -m gpu > "$OUT/tests.log" 2>&1 || { tail -30 "$OUT/tests.log"; exit 1; }
tail -3 "$OUT/tests.log"
timeout -k 10 420 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err" || { tail -20 "$OUT/bench.err"; exit 1; }
OUT="$OUT" python - <<'PY'
import json, os
d=json.loads(open(os.path.join(os.environ['OUT'], 'bench.json')).read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"])
for l in d["legs"]:
    print(l["n"], l["ms_per_step"], l["window_tables"]["window_bits_z"], l["window_tables"]["window_bits_h"], l["window_tables"]["plain_key_ms_per_proof"], l.get("throughput_in_flight",{}).get("value"), l.get("oracle_match"))
PY
