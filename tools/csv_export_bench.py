"""CSV export: the host writer (csvout.write_csv), the device path (csvout.write_csv_device) and, where it has been built, the reference converter
(oracle/_ref/csvtbin_ref -read) on one synthetic tape.

  python tools/csv_export_bench.py [--rows 5000000] [--runs 5] [--out profiles/csv_export.txt]

A nine-track NRZI tape from readtape_amd/synth.py, repeated to --rows rows (5e6 rows: 45 MB of samples, 565 MB of text), is exported
  device   one untimed run (allocations, code objects), then --runs timed runs of write_csv_device on a tensor that is resident on the device: the wall
           time to the finished file (what a user waits for: the format kernels, the copies to page-locked memory, the file system) and the kernels alone by
           HIP events on their stream - once from 1 ms (every window takes the uniform layout) and once from 2000 s (the general one: a length pass and a
           prefix sum first);
  host     --runs runs of write_csv (fprintf on one core);
  ref      one run of the reference converter on the same tape's .tbin, if oracle/_ref/csvtbin_ref is there.
The first device file is compared with the host's byte for byte before anything is timed; a difference ends the run with status 3.  Files go to a
temporary directory (--dir to choose it)."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_tape(rows):
    import numpy as np
    from readtape_amd import synth
    tape = synth.nrzi_tape(seed=9, nblocks=24, minlen=400, maxlen=800, gap_samples=4000)
    reps = -(-rows // tape.rows.shape[0])
    return tape.spec.header(), np.ascontiguousarray(np.tile(tape.rows, (reps, 1))[:rows])


def same_file(a, b):
    if os.path.getsize(a) != os.path.getsize(b):
        return False
    with open(a, "rb") as fa, open(b, "rb") as fb:
        while True:
            x, y = fa.read(1 << 24), fb.read(1 << 24)
            if x != y:
                return False
            if not x:
                return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csv_export.txt"))
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    import dataclasses
    import torch
    from readtape_amd import csvout, frontend, tbin
    be = frontend.TorchBackend()
    hdr, rows = make_tape(a.rows)
    d_rows = be.rows(rows)
    lines = [f"command: python tools/csv_export_bench.py --rows {a.rows} --runs {a.runs}",
             f"device: {torch.cuda.get_device_name(0)}; tape: {rows.shape[0]} rows x {hdr.ntrks} tracks, tdelta {hdr.tdelta_ns} ns, maxvolts {hdr.maxvolts:g}"]
    med = statistics.median
    with tempfile.TemporaryDirectory(dir=a.dir) as wd:
        host, dev = os.path.join(wd, "host.csv"), os.path.join(wd, "device.csv")
        t = time.perf_counter()
        csvout.write_csv(host, hdr, rows)
        host_wall = [time.perf_counter() - t]
        info = csvout.write_csv_device(dev, hdr, d_rows)                       # untimed: warm-up
        if not same_file(host, dev):
            print("the device path's file differs from the host's", file=sys.stderr)
            return 3
        nbytes = info["bytes"]
        lines.append(f"text: {nbytes} bytes ({nbytes / rows.shape[0]:.1f} a row); device and host files identical; files in {os.path.dirname(dev)}")
        for label, h in (("uniform", hdr), ("general", dataclasses.replace(hdr, tstart_ns=2_000_000_000_000))):
            csvout.write_csv_device(dev, h, d_rows)
            wall, fmt = [], []
            for _ in range(a.runs):
                info = csvout.write_csv_device(dev, h, d_rows)
                assert info["path"] == label, info
                wall.append(info["ms"]["total"] / 1e3)
                fmt.append(info["ms"]["format"] / 1e3)
            moved = nbytes + rows.nbytes                                      # the kernels' traffic: the text stored, the samples loaded
            lines.append(f"write_csv_device [{label}, {info['windows']} windows]: file in {med(wall):.3f} s median ({min(wall):.3f} min, {max(wall):.3f} max; "
                         f"{rows.shape[0] / med(wall) / 1e6:.2f} M rows/s, {nbytes / med(wall) / 1e9:.2f} GB/s of text); kernels alone {med(fmt) * 1e3:.2f} ms median "
                         f"({min(fmt) * 1e3:.2f} min, {max(fmt) * 1e3:.2f} max; {moved / med(fmt) / 1e9:.0f} GB/s of loads and stores)")
        for _ in range(min(a.runs, 3) - 1):                   # (three runs in all: a run is fprintf for 5e7 fields)
            t = time.perf_counter()
            csvout.write_csv(host, hdr, rows)
            host_wall.append(time.perf_counter() - t)
        lines.append(f"write_csv: file in {med(host_wall):.3f} s median ({min(host_wall):.3f} min, {max(host_wall):.3f} max; {rows.shape[0] / med(host_wall) / 1e6:.2f} M rows/s)")
        ref = os.path.join(ROOT, "oracle", "_ref", "csvtbin_ref")
        if os.path.exists(ref):
            tbin.write_tbin(os.path.join(wd, "t.tbin"), hdr, rows)
            t = time.perf_counter()
            subprocess.run([ref, "-read", "t"], cwd=wd, check=True, stdout=subprocess.DEVNULL)
            ref_wall = time.perf_counter() - t
            lines.append(f"csvtbin_ref -read: file in {ref_wall:.3f} s (one run; {rows.shape[0] / ref_wall / 1e6:.2f} M rows/s); identical to the host's: {same_file(host, os.path.join(wd, 't.csv'))}")
        else:
            lines.append("csvtbin_ref -read: not measured (oracle/_ref/csvtbin_ref is not built here)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
