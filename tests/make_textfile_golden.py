"""Writes tests/golden/text_*.npz: small hand-made SIMH .tap images (and three of the synthetic tapes), text options, and the interpreted text file the
REFERENCE writes for them (oracle/_ref/readtape_ref -tapread <options> g, and readtape_ref -textfile <options> on a .tbin; built by `make -C oracle ref`).
Run by hand where the reference is present; pytest only reads the files.

   python tests/make_textfile_golden.py

A golden holds  tap   the .tap file's bytes (-tapread) or  tape  the name of the synthetic tape (-textfile; tapout: the .tap the reference decoded from it)
                opts  the options            name  the text file's name behind "g."
                txt   the text file's bytes with the title's second line (it carries the date) cut out, and  date  that line
                status  the reference's exit status: not 0 where it stopped with a fatal error, txt then being what it had written."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import textfile_util as U  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "readtape_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def run_reference(wd, args):
    # (a path that begins with '/' is an option to the reference: run it in the file's directory on the bare name)
    p = subprocess.run([REF] + args + ["g"], cwd=wd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    names = [f for f in os.listdir(wd) if f.endswith("txt") and f.startswith("g.")]
    assert len(names) == 1, names
    txt = open(os.path.join(wd, names[0]), "rb").read()
    body, date = U.cut_date(txt)
    return p.returncode, names[0][2:], body, date


def main():
    if not os.path.exists(REF):
        sys.exit(f"{REF} is missing: make -C oracle ref")
    for name, image, opts in U.golden_cases():
        assert len(image) <= 21000, (name, len(image))
        with tempfile.TemporaryDirectory() as wd:
            open(os.path.join(wd, "g.tap"), "wb").write(image)
            status, fname, body, date = run_reference(wd, ["-tapread"] + opts)
        out = os.path.join(GOLDEN, f"text_{name}.npz")
        np.savez_compressed(out, tap=np.frombuffer(image, np.uint8), opts=np.array(opts, dtype="U40"), name=np.array(fname), txt=np.frombuffer(body, np.uint8),
                            date=np.frombuffer(date, np.uint8), status=np.array(status))
        print(f"{name}: {len(image)} bytes of .tap, {len(body)} of text, status {status}, {os.path.getsize(out)} bytes")
    import cases
    for name, (tkey, opts, extra) in sorted(U.DECODE_GOLDENS.items()):
        tape = getattr(cases, tkey)()                  # (the rows tests/golden/tape_<tkey>.npz holds)
        ref_opts = ["-v", "-tap", "-nolabels", "-nm", "-textfile"] + extra + opts
        with tempfile.TemporaryDirectory() as wd:
            tape.write(os.path.join(wd, "g.tbin"))
            status, fname, body, date = run_reference(wd, ref_opts)
            tapout = open(os.path.join(wd, "g.tap"), "rb").read()
        assert status == 0, (name, status)
        out = os.path.join(GOLDEN, f"text_{name}.npz")
        np.savez_compressed(out, tape=np.array(tkey), opts=np.array(opts, dtype="U40"), ref_opts=np.array(ref_opts, dtype="U40"), name=np.array(fname),
                            txt=np.frombuffer(body, np.uint8), date=np.frombuffer(date, np.uint8), status=np.array(status), tapout=np.frombuffer(tapout, np.uint8))
        print(f"{name}: tape {tkey}, {len(body)} bytes of text, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
