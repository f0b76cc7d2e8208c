"""Pins the CPU oracle (oracle/) against the UNMODIFIED reference compiled by oracle/Makefile:
identical SIMH .tap bytes and identical front-end event streams (track, polarity, peak time bits,
voltage bits, detection sample, AGC gain bits, baseline bits, parmset) — on fresh synthetic tapes.
Where oracle/Makefile cannot build the reference, the reference's side of every case is the one recorded in
tests/golden/ by tests/make_goldens.py - its .tap bytes, exit code and event stream of this very tape and command line
(tests/test_golden.py runs the oracle on the recorded tapes themselves)."""
import os
import subprocess

import numpy as np
import pytest

import refdump
from cases import CASES
from golden_util import load_case


def reference_opts(ref_opts):
    opts = ["-v", "-tap", "-nolabels"] + list(ref_opts)
    if "-m" not in opts:
        opts.append("-nm")
    return opts


def run_reference(ref_bin, workdir, base, ref_opts):
    opts = reference_opts(ref_opts)
    env = dict(os.environ, RT_EVENT_DUMP=os.path.join(workdir, base + ".ref.evt"))
    p = subprocess.run([ref_bin] + opts + [base], cwd=workdir, env=env, capture_output=True, text=True)
    return p


def run_oracle(oracle_bin, workdir, base, or_opts):
    p = subprocess.run([oracle_bin, "-v", f"-out={workdir}/{base}.or", f"-evt={workdir}/{base}.or.evt"] + list(or_opts)
                       + [f"{workdir}/{base}.tbin"], capture_output=True, text=True)
    return p


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_matches_reference(name, tmp_path, oracle_bin, ref_bin):
    build, ref_opts, or_opts = CASES[name]
    tape = build()
    wd = str(tmp_path)
    tape.write(os.path.join(wd, "t.tbin"))
    if getattr(build, "parms_text", ""):
        open(os.path.join(wd, "t.parms"), "w").write(build.parms_text)
        or_opts = list(or_opts) + [f"-parms={wd}/t.parms"]
    if ref_bin is not None:
        pr = run_reference(ref_bin, wd, "t", ref_opts)
        ref_tap = os.path.join(wd, "t.tap")
        ref_rc, rt = pr.returncode, (open(ref_tap, "rb").read() if os.path.exists(ref_tap) else b"")
        b = refdump.load(os.path.join(wd, "t.ref.evt"))
    else:                                            # the reference's run of this tape, as recorded
        g = load_case(name)
        sp, gh = tape.spec, g["hdr"]
        assert g["rows"].shape == tape.rows.shape and (g["rows"] == tape.rows).all(), f"{name}: the recorded tape is not this case's tape"
        assert (gh.ntrks, gh.tdelta_ns, gh.mode, gh.tstart_ns, gh.flags, gh.trkorder) == (sp.ntrks, sp.tdelta_ns, sp.mode, sp.tstart_ns, sp.flags, sp.trkorder)
        assert (np.float32([gh.maxvolts, gh.bpi, gh.ips]) == np.float32([sp.maxvolts, sp.bpi, sp.ips])).all()
        assert g["ref_opts"] == reference_opts(ref_opts) and (g["parms_text"] or "") == getattr(build, "parms_text", "")
        ref_rc, rt, b = g["returncode"], g["tap"], g["events"]
    po = run_oracle(oracle_bin, wd, "t", or_opts)
    assert po.returncode in (0, 99), po.stderr
    or_tap = os.path.join(wd, "t.or.tap")
    if ref_rc == 0:
        ot = open(or_tap, "rb").read()
        assert rt == ot, f"{name}: .tap differs"
    a = refdump.load(os.path.join(wd, "t.or.evt"))
    if ref_rc != 0:
        # the reference hit one of its own fatal asserts (exit 99): compare up to where it stopped
        n = min(a.size, b.size)
        a, b = a[:n], b[:n]
    diffs = refdump.compare(a, b)
    assert not diffs, f"{name}: " + "; ".join(diffs)
    assert a.size > 0
