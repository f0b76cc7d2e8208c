"""Randomized sweep of Whirlwind with -zeros / -differentiate -zeros / -differentiate: the device path against the CPU oracle.

Random synth.ww_tape parameters (block lengths, gaps down to a few bit times, block marks, noise, jitter, weak alternate tracks, either
polarity, heads out of line) x the three detectors x -fluxdir / -reverse / -deskew / -invert, each through oracle/_build/oracle_readtape and through
pipeline.decode_tape_ww (k_ww_det on tests/cpu_emul, or on the GPU with --gpu; a random chunk size).  The OUTCOMES are compared: the
.tap bytes and the block lines where the oracle decodes, and "both decode nothing" / "both refuse" count as agreement (-differentiate -deskew
often learns no delays and writes an empty .tap in the reference too); the summary says how many draws ended that way - a campaign in which
more than a quarter did does not count.  One process; it ends at the first device error (anything but a refusal the oracle shares).

    python tools/fuzz_ww_detectors.py [--gpu] [seed [ntapes]]          (test infrastructure; the oracle is built by readtape_amd/build.py)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from readtape_amd import pipeline, synth  # noqa: E402

ORACLE = os.path.join(ROOT, "oracle", "_build", "oracle_readtape")
DETECTORS = {"z": ["-zeros"], "dz": ["-differentiate", "-zeros"], "dp": ["-differentiate"]}


def lines(text):
    return [l.strip() for l in text.splitlines() if l.startswith("wrote block") or "tapemark at" in l or "observed flux transitions" in l or "average peak height is" in l]


def draw_tape(rng):
    kw = dict(seed=int(rng.integers(1, 1 << 30)), nblocks=int(rng.integers(1, 9)), minwords=1, maxwords=int(rng.integers(1, 20)),
              marks_every=int(rng.integers(0, 4)), gap_samples=int(rng.choice([90, 130, 200, 400, 900, 3000])), noise_mv=float(rng.choice([0, 5, 20, 50])),
              jitter=float(rng.choice([0.0, 0.02, 0.06])), amp_slope=float(rng.choice([0.02, -0.08, -0.14])), amplitude=float(rng.choice([1.3, 2.0, 3.0])))
    dsk = bool(rng.integers(0, 3) == 0)
    if dsk:
        kw["skew_cells"] = tuple(float(x) for x in rng.uniform(0, float(rng.choice([0.1, 0.35])), size=6))
    tape = synth.ww_tape(**kw)
    if rng.integers(0, 2):
        tape.rows = (-tape.rows.astype(np.int32)).clip(-32767, 32767).astype(np.int16)
    return kw, dsk, tape


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    gpu = "--gpu" in sys.argv
    seed = int(args[0]) if args else 1
    ntapes = int(args[1]) if len(args) > 1 else 20
    fe_factory = None if gpu else __import__("emul_util").emul_frontend
    rng = np.random.default_rng(seed)
    draws = mismatches = nothing = refused = 0
    combos = set()
    for i in range(ntapes):
        kw, dsk, tape = draw_tape(rng)
        fd = str(rng.choice(["neg", "pos", "auto"]))
        rev = bool(rng.integers(0, 4) == 0)
        inv = bool(rng.integers(0, 4) == 0)
        common = [f"-fluxdir={fd}"] + (["-reverse"] if rev else []) + (["-deskew"] if dsk else []) + (["-invert"] if inv else [])
        with tempfile.TemporaryDirectory() as wd:
            tape.write(os.path.join(wd, "t.tbin"))
            for det, dopts in DETECTORS.items():
                opts = dopts + common
                chunk = int(rng.choice([256, 1000, 4096]))
                q = subprocess.run([ORACLE, "-v", f"-out={wd}/o"] + opts + [os.path.join(wd, "t.tbin")], capture_output=True, text=True)
                otap = open(os.path.join(wd, "o.tap"), "rb").read() if q.returncode == 0 and os.path.exists(os.path.join(wd, "o.tap")) else b""
                olines = lines(open(os.path.join(wd, "o.log")).read()) if q.returncode == 0 else []
                msgs, err = [], None
                try:
                    pipeline.decode_tape_ww(tape.spec.header(), tape.rows, os.path.join(wd, "g.tap"), log_path=os.path.join(wd, "g.log"), fluxdir=fd, reverse=rev,
                                            deskew=dsk, invert=inv, fe_factory=fe_factory, chunk_rows=chunk, find_zeros="-zeros" in opts, differentiate="-differentiate" in opts)
                    gtap, glines = open(os.path.join(wd, "g.tap"), "rb").read(), lines(open(os.path.join(wd, "g.log")).read())
                except pipeline.ReferenceFatal as e:
                    err, refusal = e, True
                except RuntimeError as e:
                    err, refusal = e, "pre-pass found tracks without flux transitions" in str(e)
                if err is not None:
                    if refusal and q.returncode != 0:
                        refused += 1                                   # both refuse
                    elif refusal:
                        msgs.append(f"device path refused ({err}), oracle rc {q.returncode}")
                    else:                                              # a device error: the campaign ends here
                        print(f"DEVICE ERROR tape {i} {det} {kw} {opts} chunk {chunk}: {err!r}", flush=True)
                        print(f"SUMMARY seed {seed} tapes {i + 1} draws {draws + 1} combinations {len(combos)} mismatches {mismatches + 1} decoded-nothing {nothing} both-refused {refused} (stopped at a device error)", flush=True)
                        return 2
                elif q.returncode != 0:
                    msgs.append(f"oracle rc {q.returncode}, device path decoded")
                else:
                    if gtap != otap:
                        msgs.append(".tap differs")
                    if glines != olines:
                        msgs.append("block lines differ")
                    if not any(l.startswith("wrote block") or "tapemark at" in l for l in olines):
                        nothing += 1                                   # (both, if there is no message)
                draws += 1
                mismatches += bool(msgs)
                combos.add((det, fd, rev, dsk, inv))
                print(("BAD " if msgs else "ok  ") + f"{i:3d} {det:2s} rc {q.returncode} {kw} {common} chunk {chunk} blocks {len(olines)} {msgs}", flush=True)
    quarter = (nothing + refused) * 4 > draws
    print(f"SUMMARY seed {seed} tapes {ntapes} draws {draws} combinations {len(combos)} mismatches {mismatches} decoded-nothing {nothing} both-refused {refused}"
          + (" - MORE THAN A QUARTER DECODED NOTHING: this campaign does not count" if quarter else ""), flush=True)
    return 1 if mismatches or quarter else 0


if __name__ == "__main__":
    sys.exit(main())
