set -o pipefail
OUT=${OUT:-bench_out/bb}
mkdir -p "$OUT"
for B in 4096 2048; do
# --full for ttft_ms / decode_ms_per_token of the headline batch; every other extra point is switched off
timeout -k 10 500 python3 bench.py --full --batch $B --steps 2 --warmup 1 --latency-batches --no-sampled --ttft-len 0 --proxy-model '' --mp1-model '' --no-calibration --json-out "$OUT/b$B.json" > "$OUT/b$B.log" 2>&1 || { tail -20 "$OUT/b$B.log"; exit 1; }
python3 -c "
import json; d=json.load(open('$OUT/b$B.json')); print($B, d['value'], d['ttft_ms'], d['decode_ms_per_token'], d['gemm_plan_choice'])"
done
