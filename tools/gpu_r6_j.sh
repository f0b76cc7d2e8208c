#!/bin/bash
# round 6, run J: the sound kCrClear (look-ahead in k_prep, look-back in the general step): benches, the GPU tests, the shape fuzzer on the real kernels
mkdir -p runs/r06j
one() { local label=$1; shift
   env "$@" timeout 900 python bench.py --full --no-cpu-baseline --no-e2e --no-other-configs $EXTRA > runs/r06j/$label.json 2> runs/r06j/$label.err
   python - <<PY
import json
try:
    j = json.loads(open("runs/r06j/$label.json").read().strip().splitlines()[-1])
    print("$label value", j["value"], "ms", j["ms_per_step"], "serial", j["ms_per_step_serial"], "frac", j["roofline"]["frac"], "flagged", j["config"]["flagged_bursts"], "events", j["config"]["events_total"], "seq", j["config"]["last_scan_stats"]["sequential"], {k: v for k, v in j["kernel_ms"].items() if v > 0.02})
except Exception as e:
    print("$label FAILED", e); print(open("runs/r06j/$label.err").read()[-600:])
PY
}
EXTRA="--steps 20 --warmup 5" one c2 A=1
EXTRA="--config N1 --steps 5 --warmup 2" one n1 A=1
EXTRA="--config M8 --steps 5 --warmup 2" one m8 A=1
EXTRA="--config C5 --steps 5 --warmup 2" one c5 A=1
for s in 1000 1100 1200 1300; do
  timeout 900 python tools/fuzz_shapes.py --gpu $s 100 > runs/r06j/fuzz_$s.log 2>&1; echo "fuzz $s rc $? ok $(grep -c '^ok' runs/r06j/fuzz_$s.log) fail $(grep -c '^FAIL' runs/r06j/fuzz_$s.log)"
  grep -A3 '^FAIL' runs/r06j/fuzz_$s.log | head -12
done
timeout 1500 python -m pytest tests -m gpu -x -q 2>&1 | tail -3
