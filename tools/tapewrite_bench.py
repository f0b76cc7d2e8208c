"""Measures the tape writer (readtape_amd/tapewrite.py) on the GPU and prints the lines profiles/tapewrite.txt records:

  render_device   rows/s of a C2-kind NRZI tape (9 tracks, 800 BPI, records of 512 .. 4096 bytes, a tape mark every 16, gaps of 6000 rows), every row distinct,
                  by stream events: warm-up runs, then the median of --reps; and of a tape of gaps only (noise alone, no pulse is evaluated)
  render_host     the host renderer and synth.make_tape on a tape of --host-rows rows of the same kind: what the device renderer replaces
  write_tbin_device  .tap -> .tbin, wall clock, the file written under --tmp
  round trip      the resident tape decoded from HBM (pipeline.decode_tape, one parameter set as bench.py's C2): the image comes back or it does not

  python tools/tapewrite_bench.py [--rows 1e8] [--host-rows 5e6] [--reps 5] [--tmp DIR] [--skip-file] [--skip-decode]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from readtape_amd import frontend, pipeline, synth, tapewrite as W, textfile


def c2_items(target_rows, seed, spb=19.53125, gap=6000):
    """records and tape marks of bench.py's C2 kind until the tape has target_rows rows; every record its own random bytes"""
    rng = np.random.default_rng(seed)
    items, rows, n = [], gap, 0
    while rows < target_rows:
        length = int(rng.integers(512, 4097))
        items.append(("block", rng.integers(0, 256, size=length, dtype=np.int64).astype(np.uint8).tobytes()))
        rows += int(np.ceil((length + 8 + 16) * spb)) + gap
        n += 1
        if n % 16 == 0:
            items.append(("mark",))
            rows += int(np.ceil((9 + 16) * spb)) + gap
    return items


def same_image(want, got):
    a, b = textfile.read_tap(want), textfile.read_tap(got)
    if len(a) != len(b):
        return f"{len(b)} items for {len(a)}"
    for k, (x, y) in enumerate(zip(a, b)):
        if (x["kind"], x["flag"], x["length"]) != (y["kind"], y["flag"], y["length"]) or want[int(x["offset"]): int(x["offset"] + x["length"])] != got[int(y["offset"]): int(y["offset"] + y["length"])]:
            return f"item {k} differs"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--host-rows", type=float, default=5e6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--skip-file", action="store_true")
    ap.add_argument("--skip-decode", action="store_true")
    args = ap.parse_args()
    be = frontend.TorchBackend()
    torch = be.torch
    spec = W.nrzi_spec(seed=2026, gap_samples=6000)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)

    t0 = time.perf_counter()
    items = c2_items(int(args.rows), seed=7)
    image = W.tap_image(items)
    t1 = time.perf_counter()
    plan = W.encode(image, spec)
    t2 = time.perf_counter()
    nb = plan.total_rows * 18
    print(f"tape: {plan.total_rows} rows x 9 tracks ({nb / 1e9:.3f} GB of rows), {plan.blocks.size} blocks, {plan.slots.size} slots ({plan.slots.nbytes / 1e6:.1f} MB), image {len(image) / 1e6:.1f} MB; "
          f"items made in {t1 - t0:.2f} s, encoded in {t2 - t1:.3f} s", flush=True)

    def timed(p, out):
        ms = []
        for k in range(2 + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            W.render_device(p, out=out, _backend=be)
            e1.record()
            e1.synchronize()
            if k >= 2:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    rows = torch.empty((plan.total_rows, 9), dtype=torch.int16, device=be.device)
    W.device_tables(plan, be)
    med, lo, hi = timed(plan, rows)
    print(f"render_device: median {med:.2f} ms of {args.reps} (min {lo:.2f}, max {hi:.2f}) -> {plan.total_rows / med / 1e6:.3f} Grows/s, {nb / med / 1e6:.1f} GB/s of rows stored", flush=True)
    gaps = W.encode([], W.nrzi_spec(seed=2026, gap_samples=plan.total_rows))
    med_g, lo_g, hi_g = timed(gaps, rows)
    print(f"render_device, gaps only (noise, no pulses): median {med_g:.2f} ms (min {lo_g:.2f}, max {hi_g:.2f}) -> {plan.total_rows / med_g / 1e6:.3f} Grows/s, {nb / med_g / 1e6:.1f} GB/s", flush=True)
    quiet = W.encode([], W.nrzi_spec(seed=2026, gap_samples=plan.total_rows, noise_mv=0.0))
    med_q, _, _ = timed(quiet, rows)
    print(f"render_device, gaps only, noise off (the quantiser and the stores): median {med_q:.2f} ms -> {nb / med_q / 1e6:.1f} GB/s", flush=True)
    W.render_device(plan, out=rows, _backend=be)
    torch.cuda.synchronize()

    # the host renderer and synth.make_tape, on a tape a twentieth the size; and the device against the host on it
    small_items = c2_items(int(args.host_rows), seed=8)
    small = W.encode(small_items, spec)
    t0 = time.perf_counter()
    h = W.render_host(small)
    t1 = time.perf_counter()
    d = W.render_device(small, _backend=be).cpu().numpy()
    print(f"render_host: {small.total_rows} rows in {t1 - t0:.2f} s -> {small.total_rows / (t1 - t0) / 1e6:.2f} Mrows/s; device == host byte for byte: {bool(np.array_equal(h, d))}", flush=True)
    t0 = time.perf_counter()
    tape = synth.make_tape(synth.nrzi_spec(seed=2026), small_items, gap_samples=6000)
    t1 = time.perf_counter()
    print(f"synth.make_tape: {tape.rows.shape[0]} rows in {t1 - t0:.2f} s -> {tape.rows.shape[0] / (t1 - t0) / 1e6:.2f} Mrows/s", flush=True)
    del tape, h, d

    with tempfile.TemporaryDirectory(dir=args.tmp) as wd:
        if not args.skip_file:
            tap, out = os.path.join(wd, "t.tap"), os.path.join(wd, "t.tbin")
            open(tap, "wb").write(image)
            for k in range(2):                                                  # (the first run warms the page-locked buffers and the file system)
                t0 = time.perf_counter()
                r = W.write_tbin_device(tap, out, spec, _backend=be)
                dt = time.perf_counter() - t0
                print(f"write_tbin_device run {k}: {r['bytes'] / 1e9:.3f} GB in {dt:.2f} s -> {r['bytes'] / dt / 1e9:.2f} GB/s of file, {r['rows'] / dt / 1e6:.1f} Mrows/s; {r['windows']} windows, "
                      f"kernels {r['ms']['render']:.1f} ms", flush=True)
            os.remove(out)
        if not args.skip_decode:
            got = os.path.join(wd, "back.tap")
            t0 = time.perf_counter()
            stats, _ = pipeline.decode_tape(spec.header(), rows, got, opts=pipeline.DecodeOptions(multiple_tries=False))
            dt = time.perf_counter() - t0
            diff = same_image(image, open(got, "rb").read())
            print(f"round trip: {plan.total_rows} distinct rows decoded from HBM in {dt:.2f} s: {stats['blocks']} blocks, {stats['tapemarks']} tape marks, {stats['blocks_with_errors']} with errors, "
                  f"{stats['blocks_unusable']} unusable; the image came back: {diff is None}{'' if diff is None else ' (' + diff + ')'}", flush=True)


if __name__ == "__main__":
    main()
