"""Writes tests/golden/csvout_*.npz: small tapes, the converter's options, and the text the REFERENCE converter prints for them
(oracle/_ref/csvtbin_ref -read, built by `make -C oracle ref`).  Run by hand where the reference is present; pytest only reads the files.

   python tests/make_csvout_golden.py

A golden holds  tbin  the .tbin file's bytes     opts  the options behind -read     csv  the .csv file's bytes."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from readtape_amd import tbin  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "csvtbin_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def tape(seed, nrows, ntrks, amplitude=32767):
    rng = np.random.RandomState(seed)
    rows = rng.randint(-amplitude, amplitude + 1, (nrows, ntrks)).astype(np.int16)
    rows[3] = 0
    rows[4] = rows[4] % 3 - 1                       # codes -1, 0, 1: values that round to zero
    return rows


def header(ntrks=9, tdelta=1000, maxvolts=1.0, flags=tbin.FLAG_NO_REORDER, tstart=1_000_000, mode=tbin.MODE_NRZI, descr="csvout golden"):
    return tbin.TbinHeader(ntrks=ntrks, tdelta_ns=tdelta, maxvolts=maxvolts, mode=mode, bpi=800.0, ips=50.0, flags=flags, tstart_ns=tstart, descr=descr)


def cases():
    inv = tbin.FLAG_NO_REORDER | tbin.FLAG_INVERTED
    yield "plain9", header(), tape(1, 300, 9, 12000), []
    yield "inv_ties", header(tdelta=1285, flags=inv, tstart=999_999_998_000), tape(2, 150, 9, 12000), []
    yield "order7", header(ntrks=7, flags=0), tape(3, 200, 7, 12000), ["-ntrks=7", "-order=3p12045"]
    yield "stagger_ties", header(), np.zeros((40, 9), np.int16), ["-stagger=0.140625"]
    yield "stagger15", header(maxvolts=15.0), tape(4, 200, 9), ["-stagger=33.3"]
    yield "t10000", header(tdelta=333, tstart=9_999_999_999_000), tape(5, 130, 9), []
    # the window options: 300 rows from 0.001 s, 0.1 ms apart (the option parser takes times from 0.01 s)
    win = header(tdelta=100_000)
    for name, opts in (("skip", ["-skip=17"]), ("starttime", ["-starttime=0.0123"]), ("skip_starttime", ["-skip=200", "-starttime=0.0123"]),
                       ("endtime", ["-endtime=0.02"]), ("stopaft", ["-stopaft=65"]), ("start_end", ["-starttime=0.0123", "-endtime=0.0207"]),
                       ("skip_stop_end", ["-skip=5", "-stopaft=250", "-endtime=0.015"])):
        yield "win_" + name, win, tape(6, 300, 9), opts
    rail = tape(7, 100, 9)
    rail[10, 4] = rail[11, 8] = rail[12, 1] = -32768
    yield "rail_col", header(), rail, []
    yield "rail_col_inv", header(maxvolts=5.0, flags=inv), rail, []
    mid = tape(8, 120, 9)
    mid[70, 0] = -32768                             # the end mark in the middle: the text ends in front of row 70
    yield "endmark_mid", header(), mid, []


def main():
    if not os.path.exists(REF):
        sys.exit(f"{REF} is missing: make -C oracle ref")
    for name, hdr, rows, opts in cases():
        assert rows.shape[0] <= 300
        with tempfile.TemporaryDirectory() as wd:
            raw = tbin.pack_header(hdr) + np.ascontiguousarray(rows, "<i2").tobytes() + np.int16(-32768).tobytes()
            open(os.path.join(wd, "g.tbin"), "wb").write(raw)
            # (a path that begins with '/' is an option to the converter: run it in the file's directory on the bare name)
            subprocess.run([REF, "-read"] + opts + ["g"], cwd=wd, check=True, stdout=subprocess.DEVNULL)
            csv = open(os.path.join(wd, "g.csv"), "rb").read()
        out = os.path.join(GOLDEN, f"csvout_{name}.npz")
        np.savez_compressed(out, tbin=np.frombuffer(raw, np.uint8), opts=np.array(opts, dtype="U40"), csv=np.frombuffer(csv, np.uint8))
        print(f"{name}: {rows.shape[0]} rows, {csv.count(10) - 2} lines, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
