#!/bin/bash
# GPU box: rocprofv3 kernel trace + stats of a bench command (the PMC passes are tools/gpu_traffic.sh: never in one run with a trace).
# usage: tools/gpu_profile.sh <tag> [bench.py arguments, default: the driver's C2 line without the CPU legs]
# A pass that fails, faults or runs into its time limit ends the script: nothing more is started on the card behind it.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
tag=${1:-r03}; shift || true
args="$*"; [ -z "$args" ] && args="--steps 5 --warmup 2"
export TMPDIR=/tmp
out=$PWD/runs/prof_$tag
rm -rf $out; mkdir -p $out
cd /tmp
timeout -k 10 ${RTFE_PROF_TIMEOUT:-420} rocprofv3 --kernel-trace --stats -d $out/trace -o bench -- python $ROOT/bench.py --full $args --min-seconds 0 --no-cpu-baseline --no-e2e > $out/bench_under_rocprof.json 2> $out/rocprof_stderr.log
cd $ROOT
timeout -k 10 120 python tools/prof_summary.py $out "$args" > $out/summary.txt 2>&1
cat $out/summary.txt
find $out -name "*.db" -delete
