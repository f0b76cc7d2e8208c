#!/bin/bash
# GPU box, one call: the full -m gpu suite, smoke, the rocprofv3 kernel summary and the PMC traffic for C2 (and C3), the driver's bench
# line, the other configurations.  Everything lands in runs/; the builder copies the summaries to profiles/r03_*.
mkdir -p runs
timeout 1800 python -m pytest tests -m gpu -q > runs/gpu_tests.log 2>&1; echo "gpu tests rc $?"; tail -3 runs/gpu_tests.log
timeout 600 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > runs/smoke.log 2>&1; echo "smoke rc $?"; tail -1 runs/smoke.log
timeout 900 bash tools/gpu_profile.sh r03 --steps 20 --warmup 5 > runs/profile.log 2>&1; echo "profile rc $?"; head -24 runs/profile.log
timeout 900 bash tools/gpu_profile.sh r03_c3 --config C3 --steps 5 --warmup 2 > runs/profile_c3.log 2>&1; echo "profile C3 rc $?"; head -12 runs/profile_c3.log
timeout 900 bash tools/gpu_traffic.sh r03 C2 > runs/traffic.log 2>&1; echo "traffic C2 rc $?"; cp runs/traffic_r03_C2/pmc_C2.json profiles/pmc_C2.json 2>/dev/null
timeout 1500 bash tools/gpu_traffic.sh r03 C3 > runs/traffic_c3.log 2>&1; echo "traffic C3 rc $?"; cp runs/traffic_r03_C3/pmc_C3.json profiles/pmc_C3.json 2>/dev/null
timeout 900 python bench.py --full --steps 20 --warmup 5 > runs/bench_c2.json 2> runs/bench_c2.err; echo "C2 rc $?"; tail -c 2500 runs/bench_c2.json
for c in C3 C4 C5; do
  timeout 1500 python bench.py --full --config $c > runs/bench_$c.json 2> runs/bench_$c.err; echo; echo "$c rc $?"; tail -c 1400 runs/bench_$c.json
done
