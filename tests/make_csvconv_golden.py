"""Generates tests/golden/csvconv_*.npz: a CSV sample file (text), the converter's options, and the .tbin and .graph.csv the UNMODIFIED reference
converter (oracle/_ref/csvtbin_ref, compiled by oracle/Makefile) makes of it with -skip / -starttime / -endtime / -stopaft / -graph / -redo.
The redo recipe's file (a million lines: the reference's pre-read has a fixed length) is not stored: csvconv_util.redo_text makes it again from its seed,
and the golden keeps the header, the payload's sha256 and length, and the graph.  Build container only."""
import dataclasses
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import csvconv_util as U  # noqa: E402
from make_csv_golden import csv_text  # noqa: E402
from readtape_amd import synth, tbin  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "csvtbin_ref")
OUT = os.path.join(ROOT, "tests", "golden")


def text_for(name):
    """The case's text: the head of a synthetic NRZI tape, its clock set to start at 9.99 ms with a period of 1 us (so that -starttime / -endtime, which
    take 0.01 s and more, fall inside a file of a thousand lines; 12.5 ms where the start time is to lie in front of the file)."""
    nlines, ntrks, _ = U.CASES[name]
    tape = synth.nrzi_tape(seed=90 + sorted(U.CASES).index(name), nblocks=1, minlen=30, maxlen=50, gap_samples=300, ntrks=ntrks)
    spec = dataclasses.replace(tape.spec, tstart_ns=12_500_000 if name.endswith("before_t0") else 9_990_000, tdelta_ns=1000)
    assert tape.rows.shape[0] >= nlines, (name, tape.rows.shape)
    return csv_text(dataclasses.replace(tape, spec=spec, rows=tape.rows[:nlines]))


def convert(text, opts):
    """-> (.tbin bytes, .graph.csv bytes or None) of the reference."""
    with tempfile.TemporaryDirectory() as wd:
        open(os.path.join(wd, "c.csv"), "wb").write(text)
        p = subprocess.run([REF] + opts + ["c"], cwd=wd, capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        out = open(os.path.join(wd, "c.tbin"), "rb").read()
        g = os.path.join(wd, "c.graph.csv")
        return out, (open(g, "rb").read() if os.path.exists(g) else None)


def main():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
    for name, (nlines, ntrks, opts) in U.CASES.items():
        text = text_for(name).encode()
        out, graph = convert(text, opts)
        assert graph is not None
        np.savez_compressed(os.path.join(OUT, f"{name}.npz"), csv=np.frombuffer(text, dtype=np.uint8), opts=np.array(opts), tbin=np.frombuffer(out, dtype=np.uint8),
                            graph=np.frombuffer(graph, dtype=np.uint8))
        print(name, len(text), "chars ->", len(out), "bytes of .tbin,", graph.count(b"\n"), "graph lines")
    text = U.redo_text()
    for name, opts in (("csvconv_redo", U.REDO_OPTS + ["-redo"]), ("csvconv_redo_not", U.REDO_OPTS)):
        out, graph = convert(text, opts)
        _, off = tbin.parse_header(out[:4096])
        np.savez_compressed(os.path.join(OUT, f"{name}.npz"), opts=np.array(opts), csv_sha256=np.array(U.sha(text)), header=np.frombuffer(out[:off], dtype=np.uint8),
                            payload_sha256=np.array(U.sha(out[off:])), payload_bytes=np.array(len(out) - off), graph=np.frombuffer(graph, dtype=np.uint8))
        print(name, len(text), "chars ->", len(out), "bytes of .tbin, header", tbin.parse_header(out[:4096])[0].maxvolts, "V,", graph)


if __name__ == "__main__":
    main()
