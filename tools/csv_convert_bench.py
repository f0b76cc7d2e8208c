"""CSV -> TBIN, file to file: the host converter (csvin.convert_csv) and the device path (csvin.convert_csv_device) on one generated logic-analyser export.

  python tools/csv_convert_bench.py [--bytes 1000000000] [--runs 15] [--host-runs 3] [--graph 1000] [--out profiles/csv_convert.txt]

A nine-track export of about --bytes bytes (104 bytes a line; lines drawn from 2003 distinct ones, timestamps 100 ns apart) is converted with -graph=--graph
  device   one untimed run (allocations, code objects), then --runs rounds; a round is one convert_csv_device with the graph and one without, in turn: the
           wall time to the finished files, and by stream events (_timing) the upload and the index, peak, parse and graph kernels, to the microsecond;
  host     --host-runs runs of convert_csv (one core: fgets and a digit loop), one per round until they are done.
A run is a tenth of a second, so the figures that decide anything are the per-kernel event times, compared run by run, not the wall-clock medians.
The device's .tbin and .graph.csv are compared with the host's byte for byte before anything is timed; a difference ends the run with status 3."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def write_export(path, nbytes):
    import csv_shapes
    tails = [ln[ln.index(b","):] for ln in csv_shapes.plain_lines(2003, seed=77)]
    n, size = 0, 0
    with open(path, "wb") as f:
        f.write(b"".join(csv_shapes.titles()))
        while size < nbytes:
            chunk = b"".join(b"%d.%07d" % (i // 10000000, i % 10000000) + tails[(i * 7) % 2003] for i in range(n, n + 100000))
            f.write(chunk)
            n += 100000
            size += len(chunk)
    return n, os.path.getsize(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1_000_000_000)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--graph", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csv_convert.txt"))
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    import torch
    from csv_export_bench import same_file
    from readtape_amd import csvin
    med = statistics.median
    with tempfile.TemporaryDirectory(dir=a.dir) as wd:
        src, host, dev = os.path.join(wd, "e.csv"), os.path.join(wd, "host.tbin"), os.path.join(wd, "device.tbin")
        nlines, size = write_export(src, a.bytes)
        lines = [f"command: python tools/csv_convert_bench.py --bytes {a.bytes} --runs {a.runs} --host-runs {a.host_runs} --graph {a.graph}",
                 f"device: {torch.cuda.get_device_name(0)}; export: {size} bytes, {nlines} lines x 9 tracks"]
        t = time.perf_counter()
        hh, hi = csvin.convert_csv(src, host, graph=a.graph)
        host_wall = [time.perf_counter() - t]
        dh, di = csvin.convert_csv_device(src, dev, graph=a.graph)              # untimed: warm-up
        if not (same_file(host, dev) and same_file(host[:-5] + ".graph.csv", dev[:-5] + ".graph.csv") and dh == hh and di["path"] == "device"):
            print("the device path's files differ from the host's", file=sys.stderr)
            return 3
        lines.append(f".tbin: {os.path.getsize(dev)} bytes, .graph.csv: {os.path.getsize(dev[:-5] + '.graph.csv')} bytes; device and host files identical; "
                     f"{di['windows']} windows")
        # the three variants take turns, run after run, so that a drift of the machine falls on all of them alike
        labels = {f"-graph={a.graph}": a.graph, "no graph": 0}
        wall, ms = {k: [] for k in labels}, {k: [] for k in labels}
        for _ in range(a.runs):
            for label, g in labels.items():
                t = time.perf_counter()
                _, info = csvin.convert_csv_device(src, dev, graph=g, _timing=True)
                wall[label].append(time.perf_counter() - t)
                ms[label].append(info["ms"])
            if len(host_wall) < a.host_runs:
                t = time.perf_counter()
                csvin.convert_csv(src, host, graph=a.graph)
                host_wall.append(time.perf_counter() - t)
        span = lambda v: f"{med(v):.3f} median ({min(v):.3f} - {max(v):.3f})"
        for label in labels:
            parts = "; ".join(f"{k} {span([m[k] for m in ms[label]])}" for k in ("upload", "index", "peak", "parse", "graph"))
            lines.append(f"convert_csv_device [{label}], {a.runs} runs: files in {span(wall[label])} s, {size / med(wall[label]) / 1e9:.2f} GB/s of text; by stream events, ms: {parts}")
        g_label = f"-graph={a.graph}"
        graph_ms, parse_ms = [m["graph"] for m in ms[g_label]], [m["parse"] for m in ms[g_label]]
        added = [x - y for x, y in zip(wall[g_label], wall["no graph"])]
        lines.append(f"graph pass against parse pass, run by run (ms): " + ", ".join(f"{x:.3f}/{y:.3f}" for x, y in zip(graph_ms, parse_ms))
                     + f"; graph below parse in {sum(x < y for x, y in zip(graph_ms, parse_ms))} of {a.runs} runs")
        lines.append(f"wall time with the graph minus without, run by run (ms): " + ", ".join(f"{x * 1e3:+.1f}" for x in added) + f"; median {med(added) * 1e3:+.1f}")
        lines.append(f"convert_csv [-graph={a.graph}], {len(host_wall)} runs: files in {span(host_wall)} s, {size / med(host_wall) / 1e9:.3f} GB/s of text")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
