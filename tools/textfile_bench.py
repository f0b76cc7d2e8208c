"""The interpreted text dump of a large .tap three ways: the reference binary (oracle/_ref/readtape_ref -tapread, where build() has left it), the host
writer (textfile.write_text) and the device path (textfile.write_text_device); writes the three throughputs and the device run's spans to a text file.

  python tools/textfile_bench.py [--mb 256] [--record 32768] [--runs 3] [--out profiles/textfile.txt]

Method: every figure is the wall clock (time.perf_counter) of one whole call - the .tap already in the page cache, the text file written to a fresh name in
a temporary directory and left to the page cache (no fsync) - and the median of --runs calls after one untimed call; the reference runs once.  The device
run's spans are write_text_device's own: upload by the wall clock around the copy and a synchronise, format and copy-out by stream events summed over the
windows, write the writer thread's time inside the file writes; they overlap, so they do not add up to the total.  MB = 10^6 bytes of .tap image."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.path.join(ROOT, "oracle", "_ref", "readtape_ref")


def make_image(mb, record, seed=7):
    n = max(1, (mb << 20) // (record + 8))
    rng = np.random.RandomState(seed)
    img = np.zeros(n * (record + 8 + (record & 1)) + 4, np.uint8)
    v = img[:-4].reshape(n, -1)
    v[:, :4] = np.frombuffer(np.uint32(record).tobytes(), np.uint8)
    v[:, 4: 4 + record] = rng.randint(0, 256, (n, record), dtype=np.uint8)
    v[:, -4:] = v[:, :4]
    img[-4:] = 0xff
    return img, n


def body(path):
    """The file without the title's date line."""
    b = open(path, "rb").read()
    a = b.index(b"\n") + 1
    return b[:a].split(b" ", 1)[1].rsplit(b"/", 1)[-1] + b[b.index(b"\n", a) + 1:]      # (the first line names the file: without its directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--record", type=int, default=32768)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--window", type=int, default=8 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "textfile.txt"))
    a = ap.parse_args()
    from readtape_amd import frontend, textfile
    opts = textfile.TextOptions("hex", "ebcdic")
    img, nrec = make_image(a.mb, a.record)
    mbs = img.size / 1e6
    lines = [f"command: python tools/textfile_bench.py --mb {a.mb} --record {a.record} --runs {a.runs} --window {a.window}",
             f"image: {nrec} records of {a.record} bytes, {img.size} bytes of .tap; options -hex -ebcdic (32 bytes a line)",
             "method: wall clock of a whole call, file to file through the page cache, median of the runs after an untimed one (tools/textfile_bench.py's docstring)"]
    with tempfile.TemporaryDirectory() as wd:
        tap = os.path.join(wd, "g.tap")
        img.tofile(tap)

        def timed(fn, tag):
            ts, info = [], None
            for k in range(a.runs + 1):
                base = os.path.join(wd, f"{tag}{k}", "g")
                os.makedirs(os.path.dirname(base))
                t0 = time.perf_counter()
                info = fn(base)
                if k:
                    ts.append(time.perf_counter() - t0)
                if k < a.runs:
                    os.remove(textfile.text_name(base, opts))
            return ts, info, textfile.text_name(base, opts)

        ts, info, host_file = timed(lambda base: textfile.write_text(tap, base, opts, created="Tue Oct 20 12:00:00 2026"), "h")
        size = os.path.getsize(host_file)
        lines.append(f"text: {size} bytes ({size / img.size:.2f} a byte of image)")
        lines.append(f"write_text: {statistics.median(ts):.3f} s median of {len(ts)} ({min(ts):.3f} min, {max(ts):.3f} max): {mbs / statistics.median(ts):.0f} MB/s")
        want = body(host_file)
        if os.path.exists(REF):
            rd = os.path.join(wd, "r")
            os.makedirs(rd)
            os.link(tap, os.path.join(rd, "g.tap"))
            t0 = time.perf_counter()
            subprocess.run([REF, "-tapread", "-hex", "-ebcdic", "g"], cwd=rd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            t = time.perf_counter() - t0
            lines.append(f"readtape_ref -tapread: {t:.3f} s (one run): {mbs / t:.0f} MB/s; identical to the host's: {body(os.path.join(rd, 'g.hex.EBCDIC.txt')) == want}")
        else:
            lines.append("readtape_ref -tapread: not built here")
        try:
            be = frontend.TorchBackend()
        except Exception as e:
            be = None
            lines.append(f"write_text_device: no device ({type(e).__name__})")
        if be is not None:
            ts, info, dev_file = timed(lambda base: textfile.write_text_device(tap, base, opts, created="Tue Oct 20 12:00:00 2026", window_bytes=a.window, _backend=be), "d")
            m = statistics.median(ts)
            lines.append(f"write_text_device: {m:.3f} s median of {len(ts)} ({min(ts):.3f} min, {max(ts):.3f} max): {mbs / m:.0f} MB/s; identical to the host's: {body(dev_file) == want}")
            ms = info["ms"]
            lines.append(f"  last run, {info['windows']} windows: upload {ms['upload']:.1f} ms, format {ms['format']:.1f} ms, copy-out {ms['copy']:.1f} ms, write {ms['write']:.1f} ms, total {ms['total']:.1f} ms")
            lines.append(f"  format alone: {size / 1e6 / ms['format'] * 1e3:.0f} MB of text a second; copy-out: {size / 1e6 / ms['copy'] * 1e3:.0f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
