#!/bin/bash
# Round profile: the full bench JSON (--full), rocprofv3 kernel-trace stats of the plain bench step, and HBM-traffic PMC
# passes (each in its own run, no trace domains mixed in).  Summaries land in $OUT (default: out/) -> copy to profiles/.
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"; export TMPDIR=/tmp
OUT=$(mkdir -p "${OUT:-out}" && cd "${OUT:-out}" && pwd)
TAG=${1:-r01}
timeout 900 python bench.py --full > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err"; tail -c 600 "$OUT/${TAG}_bench.json"
rm -rf "$OUT/prof_$TAG"
(cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$TAG" -o $TAG -- python "$ROOT/bench.py" > "$OUT/prof_$TAG.log" 2>&1)
cp "$OUT/prof_$TAG/${TAG}_kernel_stats.csv" "$OUT/${TAG}_kernel_stats.csv" 2>/dev/null; head -8 "$OUT/${TAG}_kernel_stats.csv" | cut -c1-200
bash scripts/gpu_pmc.sh ${TAG}t "" "FETCH_SIZE" "WRITE_SIZE" "TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum TCC_EA0_RDREQ_64B_sum TCC_EA0_RDREQ_128B_sum" "TCC_EA0_WRREQ_sum TCC_EA0_WRREQ_64B_sum TCC_HIT_sum TCC_MISS_sum" > "$OUT/${TAG}_pmc_traffic.txt" 2>&1
grep -A6 "ans4s_\(enc\|dec\)_kernel\|gather" "$OUT/${TAG}_pmc_traffic.txt" | grep -v "^--" | head -60
