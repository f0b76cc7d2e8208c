"""Generates the Whirlwind -zeros / -differentiate vectors of tests/golden/ from the UNMODIFIED reference (oracle/_ref/readtape_evt,
built by oracle/Makefile), in the format of tests/make_goldens.py - the same .npz fields, the same case_<name>.npz / tape_<builder>.npz
naming - from a case table of its own.  Run in the build container only:

    python tests/make_ww_detector_goldens.py [case ...]        (no names: all cases)

Only data is stored - no reference source or text.  tests/test_golden.py finds the cases by their names and pins the CPU oracle on them."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import refdump  # noqa: E402
import cases as C  # noqa: E402
from readtape_amd import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "readtape_evt")
OUT = os.path.join(ROOT, "tests", "golden")

FAR_ZERO_PERIODS = 32768          # an event whose first exact zero lies more than 65 535 rows back: timenow - t_peak above this many sample periods


def case_ww_farzero(seed=51):
    """A noiseless tape with 70 000-row gaps and, on head 2, a +0.1 V step 1 500 rows before the second block, held for 400 rows and taken
    back over 800 rows - every decrement under the differentiator's 0.05 V dead band.  The step arms a crossing that only the block
    confirms; in between the differentiated signal is one run of exact zeros that began behind the FIRST block: the centre of the run
    lies tens of thousands of rows back, more than 16 bits of rows hold."""
    t = synth.ww_tape(seed=seed, nblocks=3, minwords=3, maxwords=8, marks_every=0, gap_samples=70000, noise_mv=0.0)
    rows = t.rows.copy()
    s2 = int(t.blocks[1][1])                                          # first row of the second block
    step = int(round(0.1 / t.spec.maxvolts * 32767))
    bump = np.zeros(rows.shape[0], dtype=np.int32)
    a = s2 - 1500
    bump[a: a + 400] = step
    bump[a + 400: a + 1200] = np.round(np.linspace(step, 0, 800, endpoint=False)).astype(np.int32)
    rows[:, 2] = (rows[:, 2].astype(np.int32) + bump).clip(-32767, 32767).astype(np.int16)
    t.rows = np.ascontiguousarray(rows)
    return t


Z, DZ, DP = ["-zeros"], ["-differentiate", "-zeros"], ["-differentiate"]
# name -> (tape builder, reference options == oracle options); every reference run also gets -v -tap -nolabels -nm (tests/make_goldens.py)
CASES = {
    "ww_z":             (C.case_ww,        Z),
    "ww_z_auto":        (C.case_ww,        Z + ["-fluxdir=auto"]),
    "ww_z_close":       (C.case_ww_close,  Z + ["-fluxdir=auto"]),
    "ww_z_rough":       (C.case_ww_rough,  Z),
    "ww_z_unused":      (C.case_ww_unused, Z + ["-fluxdir=auto"]),
    "ww_z_deskew":      (C.case_ww_skew,   Z + ["-deskew"]),
    "ww_dz":            (C.case_ww,        DZ),
    "ww_dz_pos":        (C.case_ww_pos,    DZ + ["-fluxdir=pos"]),
    "ww_dz_rough":      (C.case_ww_rough,  DZ),
    "ww_dz_close":      (C.case_ww_close,  DZ + ["-fluxdir=auto"]),
    "ww_dz_reverse":    (C.case_ww,        DZ + ["-reverse"]),
    "ww_dz_deskew":     (C.case_ww_skew,   DZ + ["-fluxdir=auto", "-deskew"]),
    "ww_dp":            (C.case_ww,        DP),
    "ww_dp_rough":      (C.case_ww_rough,  DP),
    "ww_dz_farzero":    (case_ww_farzero,  DZ),
}
MAX_BYTES = 1 << 20               # of a committed file


def main():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
    os.makedirs(OUT, exist_ok=True)
    only = set(sys.argv[1:])
    for name in sorted(CASES):
        if only and name not in only:
            continue
        build, opts_in = CASES[name]
        tape = build()
        tkey = build.__name__
        tpath = os.path.join(OUT, f"tape_{tkey}.npz")
        if not os.path.exists(tpath):                                  # (the builders of tests/cases.py: their tapes are committed)
            s = tape.spec
            np.savez_compressed(tpath, rows=tape.rows, hdr=np.array([s.ntrks, s.tdelta_ns, s.mode, s.tstart_ns, s.flags], dtype=np.int64),
                                trkorder=np.array(s.trkorder), hdrf=np.array([s.maxvolts, s.bpi, s.ips], dtype=np.float32))
        else:
            assert np.array_equal(np.load(tpath)["rows"], tape.rows), f"tape_{tkey}.npz is not what {tkey}() builds"
        with tempfile.TemporaryDirectory() as wd:
            tape.write(os.path.join(wd, "t.tbin"))
            opts = ["-v", "-tap", "-nolabels"] + list(opts_in) + ["-nm"]
            env = dict(os.environ, RT_EVENT_DUMP=os.path.join(wd, "t.evt"))
            p = subprocess.run([REF] + opts + ["t"], cwd=wd, env=env, capture_output=True, text=True)
            tap = open(os.path.join(wd, "t.tap"), "rb").read() if os.path.exists(os.path.join(wd, "t.tap")) else b""
            evt = refdump.load(os.path.join(wd, "t.evt"))
            blocks = [l.strip() for l in p.stdout.splitlines() if l.startswith("wrote block") or "tapemark at" in l or (l.startswith("  track ") and "observed flux transitions" in l) or "density was set to" in l or "average peak height is" in l]
        assert p.returncode == 0 and len(tap) > 0 and evt.size > 0, (name, p.returncode, len(tap), evt.size)
        far = ""
        if build is case_ww_farzero:
            tr = evt[evt["kind"] < 2]
            back = (tr["timenow_ns"].astype(np.float64) / 1e9 - tr["t_peak"]) / (tape.spec.tdelta_ns / 1e9)
            n = int((back > FAR_ZERO_PERIODS).sum())
            assert n >= 1, f"{name}: no event lies more than {FAR_ZERO_PERIODS} sample periods behind its confirmation (largest: {back.max():.0f})"
            far = f", {n} event(s) beyond {FAR_ZERO_PERIODS} periods (largest {back.max():.0f})"
        cpath = os.path.join(OUT, f"case_{name}.npz")
        np.savez_compressed(cpath, tape=tkey, ref_opts=np.array(opts), oracle_opts=np.array(list(opts_in), dtype="U64"),
                            tap=np.frombuffer(tap, dtype=np.uint8), events=evt, returncode=p.returncode, blocklog=np.array(blocks), parms_text=np.array(""))
        for f in (cpath, tpath):
            assert os.path.getsize(f) < MAX_BYTES, (f, os.path.getsize(f))
        print(f"{name}: {tape.rows.shape[0]} rows, {evt.size} records, tap {len(tap)} bytes, {os.path.getsize(cpath)} bytes{far}")


if __name__ == "__main__":
    main()
