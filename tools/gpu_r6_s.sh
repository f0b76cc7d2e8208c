#!/bin/bash
# round 6, run S: k_sift_hard reads the candidate's rows in aligned 16-byte pieces
mkdir -p runs/r06s
for lab in n1 n1f; do
  cfgn=$(echo $lab | sed 's/n1f/N1f/; s/^n1$/N1/')
  timeout 600 python bench.py --full --no-cpu-baseline --no-e2e --no-other-configs --config $cfgn --steps 5 --warmup 2 > runs/r06s/$lab.json 2>/dev/null
  python -c "
import json; j=json.loads(open('runs/r06s/$lab.json').read().strip().splitlines()[-1]); print('$lab', j['value'], j['ms_per_step'], j['ms_per_step_serial'], {k: v for k, v in j['kernel_ms'].items() if v > 0.02})"
done
RTFE_DEBUG=9 timeout 300 python bench.py --full --config N1 --steps 3 --warmup 1 --no-cpu-baseline --no-e2e --no-other-configs 2>/dev/null | python -c "
import json, sys
j = json.loads(sys.stdin.read().strip().splitlines()[-1]); p = j['config']['last_scan_stats']['phase_cycles']
print('k_sift_hard on N1 (RTFE_DEBUG=9), cycles of the workgroups\' first waves: fetch', p[0], 'walk', p[2], 'trips', p[3], 'workgroups', p[4], '-> per trip', p[0] // max(p[3], 1), '+', p[2] // max(p[3], 1))" | tee runs/r06s/sift_hard_phases.txt
timeout 600 python tools/fuzz_shapes.py --gpu 13000 100 > runs/r06s/fuzz.log 2>&1; echo "fuzz ok $(grep -c '^ok' runs/r06s/fuzz.log) fail $(grep -c '^FAIL ' runs/r06s/fuzz.log)"
STRESS_SHAPES=1 timeout 800 bash tools/gpu_stress.sh 3100 1 60
timeout 1800 python -m pytest tests -m gpu -x -q 2>&1 | tail -3
timeout 600 bash tools/gpu_profile.sh r06s_n1 --config N1 --steps 5 --warmup 2 --no-overlap > runs/r06s/profile_n1.log 2>&1; cp runs/prof_r06s_n1/summary.txt runs/r06s/rocprof_summary_n1.txt; cp runs/prof_r06s_n1/bench_under_rocprof.json runs/r06s/bench_under_rocprof_n1.json; head -8 runs/r06s/rocprof_summary_n1.txt
