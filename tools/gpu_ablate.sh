#!/bin/bash
OUT=${OUT:-$(mktemp -d)}; mkdir -p "$OUT"; export OUT=$(cd "$OUT" && pwd)      # this script's logs: $OUT, or a new temporary folder
cd "$(dirname "$0")/.."
for f in afterqc_amd/csrc/libafterqc_hip.so build/ablate/*.so; do
  AQC_LIB=$PWD/$f python bench.py --full --device-only --device-steps 10 --cpu-sample 0 --no-pmc "$@" > $OUT/b.log 2>$OUT/b.err
  grep PROF $OUT/b.err
  python - "$f" <<'PY'
import json, os, sys
d = json.loads(open(os.environ["OUT"] + "/b.log").read().strip().splitlines()[-1]); r = d["roofline"]
print("%-40s kernel %.4f ms  frac %.4f  qc_stat %.4f ms" % (sys.argv[1][-40:], r["kernel_ms"], r["frac"], r.get("qc_stat_kernel_ms", 0.0)))
PY
done
