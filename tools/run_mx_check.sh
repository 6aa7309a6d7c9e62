cd "$(dirname "$0")/.."; OUT="${EV_OUT:-out}"; mkdir -p "$OUT"      # logs go to $EV_OUT (default <repo>/out)
timeout 600 python -m pytest tests/test_gpu_ops.py -m gpu -q -x --timeout 300 -k "mx or attention" > "$OUT/ops_mx.log" 2>&1; echo "ops_mx rc=$?"
tail -n 5 "$OUT/ops_mx.log"
timeout 900 python -m pytest tests/test_gpu_parity.py -m gpu -q --timeout 600 -k "(mx or strict) and (golden or taps or batch_invariance or shortest)" > "$OUT/parity_mx.log" 2>&1; echo "parity_mx rc=$?"
tail -n 30 "$OUT/parity_mx.log"
timeout 600 python bench.py --full --steps 5 --warmup 2 --cpu-utts 0 --precision mx --no-other-precision --dump-launches "$OUT/launches_mx.json" > "$OUT/bench_mx.log" 2>&1; echo "bench_mx rc=$?"
OUT="$OUT" python - <<'PY'
import json, os
log = os.path.join(os.environ["OUT"], "bench_mx.log")
l=[x for x in open(log) if x.startswith("{")]
if l:
    d=json.loads(l[-1]); print(d["value"], d["ms_per_step"], d["stage_ms"]); print({k:v for k,v in d["kernels_ms"].items() if v["ms"]>0.3})
else: print(open(log).read()[-2000:])
PY
