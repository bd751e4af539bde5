# usage: bench_default.sh OUTDIR   -> OUTDIR/bench_default.json: bench.py --full (extras and CPU baselines), its headline and blocks summed up
set -o pipefail
cd "$(dirname "$0")/../.." || exit 1
OUT=${1:?usage: bench_default.sh OUTDIR}
mkdir -p "$OUT"
SECONDS=0; timeout -k 10 900 python bench.py --full > "$OUT/bench_default.json" 2> "$OUT/bench_default.err" || { tail -5 "$OUT/bench_default.err"; exit 1; }
echo "elapsed $SECONDS s"
python - "$OUT/bench_default.json" <<'PY'
import json, sys
d=json.load(open(sys.argv[1]))
print(d["value"], d["ms_per_step"], d["verified_checksums"], d["verified_ascending"], d["roofline"]["frac"], d["roofline"]["avg_launch_ms"], d["roofline"].get("traffic"))
for k,v in d.get("extra",{}).items():
    if isinstance(v,dict): print(k, v.get("value"), v.get("ms_per_step", v.get("ms_total")), v.get("verified"), v.get("error"))
print(d.get("cpu_baseline",{}).get("value"))
PY
