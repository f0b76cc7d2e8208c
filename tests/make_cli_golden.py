"""Writes tests/golden/cli_*.npz: what the REFERENCE (oracle/_ref/readtape_ref, built by `make -C oracle ref`) leaves behind for the command lines of
tests/cli_util.py's RUNS - the names and bytes of its output files (a text file without its date line) and the lines of its log that the tests compare.
Run by hand where the reference is present; pytest only reads the files.

   python tests/make_cli_golden.py

A golden holds  tape   the name of the tape in cli_util.TAPES, and  crc  the CRC of its rows
                opts   the options               names, file<i>   the output files            log   cli_util.log_lines of g.log"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cli_util as U  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "readtape_ref")


def main():
    if not os.path.exists(REF):
        sys.exit(f"{REF} is missing: make -C oracle ref")
    for name, (tname, opts) in sorted(U.RUNS.items()):
        t = U.tape(tname)
        with tempfile.TemporaryDirectory() as wd:
            t.write(os.path.join(wd, "g.tbin"))
            p = subprocess.run([REF] + opts + ["g"], cwd=wd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            assert p.returncode == 0, (name, p.returncode)
            files = U.output_files(wd)
            log = U.log_lines(open(os.path.join(wd, "g.log")).read())
        if tname in U.LABEL_TAPES and "-tap" not in opts and "-nolabels" not in opts:
            # (a tape the reference does not see labels on never becomes a fixture)
            assert any(re.fullmatch(r"g-001-[A-Z]+\.bin", f) for f in files), (name, sorted(files))
            assert any(l.startswith("*** tape label HDR1") for l in log), name
        names = sorted(files)
        out = os.path.join(U.GOLDEN, f"cli_{name}.npz")
        np.savez_compressed(out, tape=np.array(tname), crc=np.array(U.rows_crc(t), np.int64), opts=np.array(opts, dtype="U60"), names=np.array(names, dtype="U80"),
                            log=np.array(log, dtype="U300"), **{f"file{i}": np.frombuffer(files[n], np.uint8) for i, n in enumerate(names)})
        print(f"{name}: {tname} {' '.join(opts)} -> {', '.join(f'{n} ({len(files[n])})' for n in names)}; {len(log)} log lines, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
