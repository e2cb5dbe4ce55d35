#!/bin/bash
# split-bf16 vs fp32 end to end, short: prints value / lanes / group / stage times of each
# usage: tools/probes/bench_pair.sh [output directory, default probe_out]
OUT=${1:-probe_out}
mkdir -p "$OUT"
for mm in 1 0; do
  python bench.py --full --steps 32 --warmup 3 --repeats 3 --sustain-seconds 0 --no-cpu-baseline --no-host-input-leg --no-alt-pass --math-mode $mm > "$OUT/bp_$mm.log" 2>&1
  grep '^{' "$OUT/bp_$mm.log" | tail -1 > "$OUT/bp_$mm.json"
  python - $mm "$OUT" <<'P'
import json, os, sys
mm, out = sys.argv[1], sys.argv[2]
try:
    d = json.load(open(os.path.join(out, "bp_%s.json" % mm)))
except Exception as e:
    print("math mode", mm, "no JSON line:", e); print(open(os.path.join(out, "bp_%s.log" % mm)).read()[-1500:]); sys.exit(0)
print("math mode", mm, "value %.1f" % d["value"], "lanes", d["lanes"], "group", d["group"], ["%.1f" % v for v in d["repeats"]["images_per_s"]], d["config"]["gather"])
print("   serial stage ms", {k: round(v, 3) for k, v in d["stage_ms_serial_image"].items()})
print("   single-image latency ms", d["roofline"].get("single_image_mode", {}).get("latency_ms"))
P
done
