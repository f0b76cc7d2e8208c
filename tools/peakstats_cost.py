"""What decode_tape(peakstats=True) costs (profiles/peakstats.txt, "on against off"): one resident NRZI tape of the benchmark's C2 kind (bench.make_base_tape, four
copies of the 5e6-row base tape) through pipeline.decode_tape with peakstats False and True, alternating, after one untimed decode.  Timed from the scan's fetch
(from its start, and from its end) to decode_tape's return: the host replay with the histogram update on every recorded transition, the statistics file and the
verdict included - the device scan is the same either way.

   python tools/peakstats_cost.py [--runs 8] [--copies 4]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from readtape_amd import frontend, pipeline  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8, help="timed decodes (half of them with peakstats)")
    ap.add_argument("--copies", type=int, default=4)
    args = ap.parse_args()
    tape = bench.make_base_tape(seed=1000, target_rows=5e6, kind="nrzi")
    hdr = tape.spec.header()
    rows = np.tile(tape.rows, (args.copies, 1))
    marks = {}
    real = frontend.ScanResult.fetch

    def fetch(self, *a, **k):
        first = "start" not in marks                  # (the scan's own fetch, not an exact rescan's inside the replay)
        if first:
            marks["start"] = time.perf_counter()
        r = real(self, *a, **k)
        if first:
            marks["end"] = time.perf_counter()
        return r
    frontend.ScanResult.fetch = fetch
    runs = []
    with tempfile.TemporaryDirectory() as wd:
        for i in range(args.runs + 1):
            on = bool(i % 2) if i else False          # run 0: untimed, off
            marks.clear()
            st, _ = pipeline.decode_tape(hdr, rows, os.path.join(wd, f"t{i}.tap"), opts=pipeline.DecodeOptions(verbose=False), peakstats=on)
            t = time.perf_counter()
            rec = dict(run=i, peakstats=on, fetch_start_to_return=round(t - marks["start"], 4), fetch_end_to_return=round(t - marks["end"], 4),
                       events=int(st["events_delivered"]), blocks=int(st["blocks"]), attempts=int(st["attempts"]), exact_scans=int(st["exact_scans"]))
            if on:
                rec["measurements"] = int(st["peakstats"]["counts"].sum())
            print(json.dumps(rec), flush=True)
            if i:
                runs.append(rec)
    out = {"rows": int(rows.shape[0])}
    for key in ("fetch_start_to_return", "fetch_end_to_return"):
        off = float(np.median([r[key] for r in runs if not r["peakstats"]]))
        on = float(np.median([r[key] for r in runs if r["peakstats"]]))
        out[key] = dict(off_median_s=round(off, 4), on_median_s=round(on, 4), ratio=round(on / off, 4))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
