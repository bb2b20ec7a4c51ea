#!/bin/bash
# rocprofv3 kernel-trace stats of the default bench + chunk-size sweep -> $OUT (default: out/)
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"; export TMPDIR=/tmp
OUT=$(mkdir -p "${OUT:-out}" && cd "${OUT:-out}" && pwd)
TAG=${1:-r01}
timeout 900 python -m pytest tests -x -q -m gpu > "$OUT/pytest_gpu.log" 2>&1; echo "pytest rc=$?"; tail -3 "$OUT/pytest_gpu.log"
for c in 512 1024 2048 4096 8192; do
  timeout 300 python bench.py --full --steps 10 --warmup 2 --chunk $c --no-cpu 2>/dev/null | tail -1 > "$OUT/bench_chunk$c.json"
  python - <<PY
import json; r=json.load(open("$OUT/bench_chunk$c.json")); print("chunk",$c,"value",r["value"],"enc",r["enc_MBps"],"dec",r["dec_MBps"],"ratio",r["config"]["ratio"],"ms",r["ms_per_step"], r["roofline"]["enc_kernel_ms"], r["roofline"]["dec_kernel_ms"])
PY
done
rm -rf "$OUT/prof_$TAG"
(cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$TAG" -o $TAG -- python "$ROOT/bench.py" --steps 10 --warmup 2 > "$OUT/prof_$TAG.log" 2>&1)
find "$OUT/prof_$TAG" -name "*stats*" | head
f=$(find "$OUT/prof_$TAG" -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -12 "$f"
