#!/bin/bash
# rocprofv3 kernel stats + bench --full line for every secondary coder at the bench chunk -> $OUT/r02_codec_* (default: out/)
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"; export TMPDIR=/tmp
OUT=$(mkdir -p "${OUT:-out}" && cd "${OUT:-out}" && pwd)
for cdc in ${1:-rccdfs rccdfsm rccdfs2 rccdf rccdfi anscdf anscdf1 rcs rccdf4 rccdf4i anscdf4}; do
  rm -rf "$OUT/prof_$cdc"
  (cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$cdc" -o $cdc -- python "$ROOT/bench.py" --steps 5 --warmup 1 --codec $cdc > "$OUT/prof_$cdc.log" 2>&1)
  cp "$OUT/prof_$cdc/${cdc}_kernel_stats.csv" "$OUT/r02_codec_${cdc}_kernel_stats.csv"
  timeout 300 python bench.py --full --no-cpu --steps 10 --warmup 2 --codec $cdc 2>/dev/null | tail -1 > "$OUT/r02_codec_${cdc}_bench.json"
  python -c "
import json,csv
r=json.load(open('$OUT/r02_codec_${cdc}_bench.json')); print('$cdc', r['value'], 'enc', r['enc_MBps'], 'dec', r['dec_MBps'], r['config']['ratio'])
for x in list(csv.DictReader(open('$OUT/r02_codec_${cdc}_kernel_stats.csv')))[:4]: print('   ', x['Name'][:44], x['Calls'], x['AverageNs'])"
done
