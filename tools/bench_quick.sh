#!/bin/bash
# the full bench line (north-star record included), no CPU baseline. Usage: bash tools/bench_quick.sh TAG
# (the log goes to $OUT_ROOT/TAG/bench.log, OUT_ROOT defaults to bench_out)
OUT=${OUT_ROOT:-bench_out}/$1
mkdir -p "$OUT"
timeout -k 10 500 python -u bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > "$OUT/bench.log" 2>&1; echo "bench rc=$?"
grep '^{"metric"' "$OUT/bench.log" | python3 -c "
import json,sys
d=json.loads(sys.stdin.read())
ns=d.get('north_star') or {}
print('value', d['value'], 'ms', d['ms_per_step'], 'ns', ns.get('value'), ns.get('ms_per_step'))
for k,v in d['roofline'].get('by_kernel',{}).items(): print(' ', k, v['launch_ms'], v['tflops'], v['frac'])
"
