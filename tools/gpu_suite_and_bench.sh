#!/usr/bin/env bash
# GPU suite, smoke, then the bench with every extra point (bench.py --full): $OUT/{pytest.log,smoke.log,bench.json},
# OUT = bench_out/suite unless set
set -o pipefail
OUT=${OUT:-bench_out/suite}
mkdir -p "$OUT"
timeout -k 10 900 python3 -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > "$OUT/pytest.log" 2>&1 || { tail -40 "$OUT/pytest.log"; exit 1; }
tail -2 "$OUT/pytest.log"
timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || { tail -20 "$OUT/smoke.log"; exit 1; }
tail -2 "$OUT/smoke.log"
if [ "${BENCH:-1}" = 1 ]; then
  timeout -k 10 900 python3 bench.py --full --json-out "$OUT/bench.json" > "$OUT/bench.log" 2>&1 || { tail -20 "$OUT/bench.log"; exit 1; }
  python3 -c "
import json; d=json.load(open('$OUT/bench.json'))
print('value', d['value'], 'ttft', d['ttft_ms'], 'decode', d['decode_ms_per_token'])
print('lat', [p['decode_ms_per_token'] for p in d['latency_points']['points']])
print('proxy', [p['decode_ms_per_token'] for p in d['tp_rank_proxy']['points']])
print('mp1', d.get('mp1_point', {}).get('point', {}).get('decode_ms_per_token'))
print('ttft2048', d.get('ttft'))
print('cal', d.get('calibration'))
"
fi
