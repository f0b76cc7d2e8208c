"""Writes tests/golden/peakstats_*.npz: the flux-transition statistics files the REFERENCE (oracle/_ref/readtape_ref, built by `make -C oracle ref`) leaves
behind for the command lines of tests/peakstats_util.py's RUNS - <base>.peakstats.csv and, after -deskew, <base>.peakstats_deskew.csv - and the lines of its
log about them and about the head skew.  Run by hand where the reference is present; pytest only reads the files.

   python tests/make_peakstats_golden.py

A golden holds  tape   the name of the tape in peakstats_util.TAPES, and  crc  the CRC of its rows
                opts   the options               names, file<i>   the statistics files        log   peakstats_util.peak_lines of g.log"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cli_util  # noqa: E402
import peakstats_util as U  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "readtape_ref")


def main():
    if not os.path.exists(REF):
        sys.exit(f"{REF} is missing: make -C oracle ref")
    for name, (tname, opts) in sorted(U.RUNS.items()):
        t = U.tape(tname)
        with tempfile.TemporaryDirectory() as wd:
            t.write(os.path.join(wd, "g.tbin"))
            if name in U.PARMS:
                open(os.path.join(wd, "g.parms"), "w").write(U.PARMS[name])
            p = subprocess.run([REF] + opts + ["g"], cwd=wd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            assert p.returncode == 0, (name, p.returncode)
            files = U.peak_files(wd)
            log = U.peak_lines(open(os.path.join(wd, "g.log")).read())
        quiet = "-q" in opts
        assert ("g.peakstats.csv" in files) == (not quiet), (name, sorted(files))
        assert all(len(d) < 8192 and d.count(b"\n") >= 6 for d in files.values()), name
        names = sorted(files)
        out = os.path.join(U.GOLDEN, f"peakstats_{name}.npz")
        np.savez_compressed(out, tape=np.array(tname), crc=np.array(cli_util.rows_crc(t), np.int64), opts=np.array(opts, dtype="U60"), names=np.array(names, dtype="U80"),
                            log=np.array(log, dtype="U300"), **{f"file{i}": np.frombuffer(files[n], np.uint8) for i, n in enumerate(names)})
        print(f"{name}: {tname} {' '.join(opts)} -> {', '.join(f'{n} ({len(files[n])})' for n in names)}; {len(log)} log lines, {os.path.getsize(out)} bytes")
        for l in log:
            print("     " + l)


if __name__ == "__main__":
    main()
