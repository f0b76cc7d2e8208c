"""CSV ingest: the host loader (csvin.read_csv) against the device path (csvin.read_csv_device) on one synthetic export.

  python tools/gpu_csv_time.py [--rows 2000000] [--ntrks 9] [--runs 5] [--out profiles/csv_device.txt]

Synthesises a rows x ntrks CSV (2e6 x 9: about 210 MB) into a temporary directory, reads it once so that it sits in the page cache, then runs three steps,
each a process of its own under `timeout -k 10`, each started only if the one before ended well (nothing is started after a fault):
  compare   both loaders once: headers, every code, clip counts and columns must be identical
  host      `runs` timed runs of read_csv (wall time)
  device    one untimed run (allocations), then `runs` timed runs of read_csv_device: wall time (synchronised), and the upload and the three kernels'
            launches (rtfe_csv_index, _peak, _parse) by HIP events on their stream
and writes medians and minima, bytes, rows/s, and the kernels' share of the wall time to --out.  Exit status 0: outputs identical AND the device
path's median below the host path's minimum."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthesise(path, rows, ntrks):
    import numpy as np
    rng = np.random.RandomState(11)
    k = 4099
    v = 2.5 * np.sin(0.41 * np.arange(k)[:, None] + np.arange(ntrks)[None, :]) + rng.uniform(-0.2, 0.2, (k, ntrks))
    tails = [(", " + ", ".join(f"{x:.6f}" for x in r) + "\n").encode() for r in v]
    with open(path, "wb") as f:
        f.write(b"synthetic export\n" + ("Time [s], " + ", ".join(f"c{i}" for i in range(ntrks)) + "\n").encode())
        for i0 in range(0, rows, 1 << 16):
            f.write(b"".join(b"%d.%07d" % (i // 10000000, i % 10000000) + tails[(i * 5) % k] for i in range(i0, min(i0 + (1 << 16), rows))))
    return os.path.getsize(path)


def step_compare(a):
    import numpy as np
    from readtape_amd import csvin
    h0, r0, i0 = csvin.read_csv(a.path, ntrks=a.ntrks)
    h1, r1, i1 = csvin.read_csv_device(a.path, ntrks=a.ntrks)
    r1 = r1.cpu().numpy()
    same = h0 == h1 and r0.shape == r1.shape and bool(np.array_equal(r0, r1)) and all(i0[k] == i1[k] for k in i0) and i1["path"] == "device"
    json.dump(dict(identical=same, rows=int(r0.shape[0]), windows=i1["windows"], clipped=i1["clipped_samples"], maxvolts=h1.maxvolts, tdelta_ns=h1.tdelta_ns), open(a.result, "w"))
    return 0 if same else 3


def step_host(a):
    from readtape_amd import csvin
    wall = []
    for _ in range(a.runs):
        t = time.perf_counter()
        csvin.read_csv(a.path, ntrks=a.ntrks)
        wall.append(time.perf_counter() - t)
    json.dump(dict(wall=wall), open(a.result, "w"))
    return 0


def step_device(a):
    import torch
    from readtape_amd import csvin
    csvin.read_csv_device(a.path, ntrks=a.ntrks)
    torch.cuda.synchronize()
    wall, ms = [], []
    for _ in range(a.runs):
        t = time.perf_counter()
        _, rows, _ = csvin.read_csv_device(a.path, ntrks=a.ntrks)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t)
        del rows
    for _ in range(a.runs):                      # (the events in runs of their own: the wall times above carry none)
        _, rows, info = csvin.read_csv_device(a.path, ntrks=a.ntrks, _timing=True)
        ms.append(info["ms"])
        del rows
    json.dump(dict(wall=wall, ms=ms, device=torch.cuda.get_device_name(0)), open(a.result, "w"))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2000000)
    ap.add_argument("--ntrks", type=int, default=9)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csv_device.txt"))
    ap.add_argument("--step")
    ap.add_argument("--path")
    ap.add_argument("--result")
    a = ap.parse_args()
    if a.step:
        return dict(compare=step_compare, host=step_host, device=step_device)[a.step](a)
    with tempfile.TemporaryDirectory() as wd:
        path = os.path.join(wd, "synthetic.csv")
        nbytes = synthesise(path, a.rows, a.ntrks)
        with open(path, "rb") as f:
            while f.read(1 << 24):
                pass
        res = {}
        for step, limit in (("compare", 300), ("host", 300), ("device", 300)):
            out = os.path.join(wd, step + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--path", path, "--result", out,
                                 "--ntrks", str(a.ntrks), "--runs", str(a.runs)]).returncode
            if rc != 0:
                print(f"step {step} ended with status {rc}: nothing further is started", file=sys.stderr)
                return rc
            res[step] = json.load(open(out))
    med, mn = statistics.median, min
    hw, dw = res["host"]["wall"], res["device"]["wall"]
    keys = ("upload", "index", "peak", "parse")
    kms = {k: [m[k] for m in res["device"]["ms"]] for k in keys}
    kern = [m["index"] + m["peak"] + m["parse"] for m in res["device"]["ms"]]
    ok = res["compare"]["identical"] and med(dw) < mn(hw)
    lines = [f"tools/gpu_csv_time.py --rows {a.rows} --ntrks {a.ntrks} --runs {a.runs}   ({res['device']['device']})",
             f"file: {nbytes} bytes, {res['compare']['rows']} rows x {a.ntrks} tracks, {res['compare']['windows']} window(s); outputs identical: {res['compare']['identical']}"
             f" (maxvolts {res['compare']['maxvolts']:.1f}, tdelta {res['compare']['tdelta_ns']} ns, clipped {res['compare']['clipped']})",
             f"read_csv         wall s: median {med(hw):.4f}  min {mn(hw):.4f}   {res['compare']['rows'] / med(hw) / 1e6:.2f} M rows/s  {nbytes / med(hw) / 1e6:.0f} MB/s",
             f"read_csv_device  wall s: median {med(dw):.4f}  min {mn(dw):.4f}   {res['compare']['rows'] / med(dw) / 1e6:.2f} M rows/s  {nbytes / med(dw) / 1e6:.0f} MB/s",
             f"host minimum / device median: {mn(hw) / med(dw):.1f}"]
    for k in keys:
        lines.append(f"  {'upload (pinned -> device)' if k == 'upload' else 'rtfe_csv_' + k:28s} ms: median {med(kms[k]):.3f}  min {mn(kms[k]):.3f}")
    lines.append(f"  the three kernels' launches   ms: median {med(kern):.3f}  min {mn(kern):.3f} = {100 * med(kern) / 1e3 / med(dw):.1f} % of the device path's median wall time")
    lines.append(f"condition (outputs identical, device median < host minimum): {'met' if ok else 'NOT met'}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text, end="")
    return 0 if ok else 4


if __name__ == "__main__":
    sys.exit(main())
