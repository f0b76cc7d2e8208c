"""Shape fuzzer for the peak path's record logic (k_sift / k_prep / k_gain), on the CPU emulator against the oracle.

Gaussian noise (tools/gpu_stress.sh, the N1 tape) almost never draws the shapes that decide whether a record may fire on the lean step:
two extremes of nearly the same height inside one window, a narrow valley right behind a flat top, a notch in a shoulder.  This tool
writes such shapes over peaks of a clean NRZI tape - every sample of the window either side of a chosen peak drawn from a mixture of
"a hair below the peak", "a little below", "well below" - and checks every event against the oracle.

  python tools/fuzz_shapes.py [--gpu] [--e2e] [seed0 [ntapes [kind]]]     (test infrastructure: the oracle through tests/parity_util; without --gpu the kernels run on tests/cpu_emul)
  python tools/fuzz_shapes.py [--gpu] --zeros | --diffz [seed0 [ntapes]]   (-zeros / -zeros -differentiate: tests/zeros_shapes.py's tapes end to end against the oracle;
                                                                            --diffz: tests/diffz_util.py's classes on k_diffz's seams as well, every third tape with
                                                                            -invert, every third with a deskew delay of 50, and k_diffz against k_decode byte for byte)
  python tools/fuzz_shapes.py [--gpu] --rails [seed0 [ntapes]]             (the int16 rails on the amplitude detectors: tests/rail_shapes.py's tapes, every event field and the .tap
                                                                            against the oracle; stops at the first mismatch or failure)
  python tools/fuzz_shapes.py [--gpu] --seams [seed0 [ntapes]]             (the amplitude shapes ON the seams of the peak and dense paths: tests/seam_shapes.py's tapes, every event field
                                                                            against the oracle, two scans a handle; a line per tape with what its shapes lay across and - on the
                                                                            emulator - what its segments met (seg_shapes:); stops at the first mismatch or failure)
  python tools/fuzz_shapes.py [--gpu] --pe [seed0 [ntapes]]                (where a PE preamble ends: tests/pe_shapes.py's classes - a draw is a class, a seed, -invert, a -skew= list,
                                                                            -m and a path - every event field against the oracle, two scans a handle; a line per tape with what
                                                                            the oracle says it contains (classes_met) and the totals at the end; stops at the first mismatch or failure)
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fuzz_util import KINDS, draw, shape_tape  # noqa: E402,F401


def main():
    from parity_util import check_tape, config_for, oracle_attempts
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    gpu = "--gpu" in sys.argv
    seed0 = int(args[0]) if len(args) > 0 else 1
    ntapes = int(args[1]) if len(args) > 1 else 4
    only = args[2] if len(args) > 2 else None          # one of KINDS: every tape of that format
    if gpu:
        from readtape_amd import frontend
        make = frontend.FrontEnd
    else:
        from emul_util import emul_frontend
        make = emul_frontend
    if "--zeros" in sys.argv or "--diffz" in sys.argv:
        return zeros_main(make, gpu, seed0, ntapes, diff="--diffz" in sys.argv)
    if "--rails" in sys.argv:
        return rails_main(make, seed0, ntapes)
    if "--seams" in sys.argv:
        return seams_main(make, gpu, seed0, ntapes)
    if "--pe" in sys.argv:
        return pe_main(make, seed0, ntapes)
    bad = 0
    for seed in range(seed0, seed0 + ntapes):
        d = draw(seed)
        if only:
            d["kind"] = only
        tape, rows, nsites, opts = shape_tape(seed, **d)
        hdr = tape.spec.header()
        with tempfile.TemporaryDirectory() as td:
            att = oracle_attempts(hdr, rows, opts, td)
        fe = make(config_for(hdr, opts))
        if "--e2e" in sys.argv:                                  # the whole pipeline on the shaped tape - front end, host decoders, .tap writer - against the oracle's .tap and its transitions
            import subprocess
            import refdump
            from parity_util import ORACLE
            from readtape_amd import pipeline, tbin
            with tempfile.TemporaryDirectory() as wd:
                tbin.write_tbin(os.path.join(wd, "t.tbin"), hdr, rows)
                p = subprocess.run([ORACLE, "-v", f"-out={wd}/o", f"-evt={wd}/o.evt"] + opts + [os.path.join(wd, "t.tbin")], capture_output=True, text=True)
                st, _ = pipeline.decode_tape(hdr, rows, os.path.join(wd, "g.tap"), evt_path=os.path.join(wd, "g.evt"), opts=pipeline.DecodeOptions(multiple_tries="-m" in opts), fe_factory=None if gpu else make)
                a, b = refdump.load(os.path.join(wd, "g.evt")), refdump.load(os.path.join(wd, "o.evt"))
                m2 = refdump.compare(a, b)
                if p.returncode == 0 and open(os.path.join(wd, "g.tap"), "rb").read() != open(os.path.join(wd, "o.tap"), "rb").read():
                    m2.append(".tap differs")
                print(f"{'ok' if not m2 else 'FAIL'} seed {seed} {d} e2e: {a.size} transitions, oracle rc {p.returncode}", flush=True)
                if m2:
                    bad += 1
                    print("\n".join(str(x) for x in m2[:6]), flush=True)
        for rep in range(2):                                    # (the second scan runs under the floor the first one learned)
            msgs, stats = check_tape(fe, hdr, rows, att)
            st = fe.scan_stats(fe.scan(rows).fetch())
            print(f"{'ok' if not msgs else 'FAIL'} seed {seed} {d} rep {rep} sites {nsites} events {stats['events']} exact {stats['exact']} parallel {st['parallel']} sequential {st['sequential']} redone {st['redone']} gave_up {st['gave_up']}", flush=True)
            if msgs:
                bad += 1
                print("\n".join(msgs[:6]), flush=True)
    print("FAILURES", bad)
    return 1 if bad else 0


def zeros_main(make, gpu, seed0, ntapes, diff):
    import zeros_shapes as zs
    from readtape_amd import frontend

    def bursts(hdr, rows):
        return make(frontend.FrontEndConfig.from_header(hdr, find_zeros=True)).scan(rows).fetch(events=False).bursts
    bad = 0
    if diff:
        return diffz_main(make, gpu, seed0, ntapes)
    for seed in range(seed0, seed0 + ntapes):
        hdr, rows0, rows, sites, opts = zs.shaped(seed, bursts, diff=diff)
        if seed % 4 == 3 and not diff:
            opts = opts + ["-invert"]                          # (k_decode's zero-crossing mode)
        with tempfile.TemporaryDirectory() as wd:
            msgs, b = zs.e2e(hdr, rows, opts, wd, None if gpu else make)
        cov = zs.coverage(sites, hdr, rows.shape[0], bursts(hdr, rows))
        print(f"{'ok' if not msgs else 'FAIL'} seed {seed} {zs.draw(seed)} {' '.join(opts)} sites {len(sites)} transitions {b.size} "
              f"seams {sum(cov.get(c, 0) for c in zs.SEAMS)}", flush=True)
        if msgs:
            bad += 1
            print("\n".join(str(x) for x in msgs[:6]), flush=True)
    print("FAILURES", bad)
    return 1 if bad else 0


def diffz_main(make, gpu, seed0, ntapes):
    """k_diffz: a shaped tape a seed end to end against the oracle, and its scan against k_decode's (RTFE_DIFFZ_KERNEL=0) byte for byte"""
    import diffz_util as dz
    import zeros_shapes as zs
    import zeros_util
    from readtape_amd import frontend
    if not gpu:
        make = dz.emul_frontend

    def bursts(hdr, rows, **kw):
        return make(frontend.FrontEndConfig.from_header(hdr, find_zeros=True, **kw)).scan(rows).fetch(events=False).bursts
    bad = 0
    for seed in range(seed0, seed0 + ntapes):
        hdr, rows0, rows, sites, opts = dz.shaped(seed, bursts)
        kw = {}
        if seed % 3 == 1:
            opts, kw = opts + ["-invert"], {"invert": True}
        if seed % 3 == 2:
            opts, kw = opts + [dz.skew_opt(hdr.ntrks, seed)], {"skew": [int(x) for x in dz.skew_opt(hdr.ntrks, seed)[6:].split(",")]}
        with tempfile.TemporaryDirectory() as wd:
            msgs, b = zs.e2e(hdr, rows, opts, wd, None if gpu else make)
        res = []
        for knob in (None, "0"):
            os.environ.pop(dz.KNOB, None)
            if knob is not None:
                os.environ[dz.KNOB] = knob
            res.append(make(frontend.FrontEndConfig.from_header(hdr, find_zeros=True, differentiate=True, **kw)).scan(rows).fetch())
        os.environ.pop(dz.KNOB, None)
        try:
            zeros_util.same_scan(res[1], res[0], hdr.ntrks)
        except AssertionError as e:
            msgs = msgs + [f"k_diffz against k_decode: {e!r}"]
        cov = dz.coverage(sites, hdr, rows.shape[0], res[0].bursts)
        print(f"{'ok' if not msgs else 'FAIL'} seed {seed} {zs.draw(seed)} spb {dz.spb_of(hdr)} {' '.join(opts)} sites {len(sites)} transitions {b.size} events {int(res[0].counts.sum())} "
              + " ".join(f"{c} {cov.get(c, 0)}" for c in dz.NEW_SHAPES + dz.SEAMS), flush=True)
        if msgs:
            bad += 1
            print("\n".join(str(x) for x in msgs[:6]), flush=True)
    print("FAILURES", bad)
    return 1 if bad else 0


def rails_main(make, seed0, ntapes):
    """tests/test_emul_rails.py's check of one shaped tape per seed; the first tape that fails ends the run (no retries: what failed is looked at, not run again)"""
    import rail_shapes as rs
    from test_emul_rails import shaped_case
    for seed in range(seed0, seed0 + ntapes):
        with tempfile.TemporaryDirectory() as wd:
            try:
                d, cov = shaped_case(make, seed, wd)
            except Exception as e:                              # a mismatch (AssertionError) or a failure of the front end
                print(f"FAIL seed {seed} {rs.draw(seed)}: {type(e).__name__}: {str(e)[:2000]}", flush=True)
                print("FAILURES 1 (stopped at the first)")
                return 1
        print(f"ok seed {seed} {d} shapes {sum(cov.get(c, 0) for c in rs.SHAPES)} rail samples on seams {sum(cov.get(c, 0) for c in rs.SEAMS)}", flush=True)
    print("FAILURES 0")
    return 0


def seams_main(make, gpu, seed0, ntapes):
    """tests/seam_util.py's check of one shaped tape per seed (seam_tape); the first tape that fails ends the run (no retries)"""
    import seam_shapes as ss
    from seam_util import seam_tape
    if not gpu:
        os.environ["RTFE_PREP_CHECK"] = "2"
    nfast = 0
    for seed in range(seed0, seed0 + ntapes):
        d = ss.draw(seed)
        hdr, rows0, rows, sites, opts = ss.shaped(seed)
        sys.stderr.flush()
        with tempfile.TemporaryDirectory() as wd, tempfile.TemporaryFile() as errf:
            keep = os.dup(2)
            os.dup2(errf.fileno(), 2)                            # (the emulator's kernels print to the C stderr)
            try:
                stats, st, att = seam_tape(make, hdr, rows, opts, wd)
                fail = None
            except Exception as e:                               # a mismatch (AssertionError) or a failure of the front end
                fail = f"{type(e).__name__}: {str(e)[:2000]}"
            finally:
                os.dup2(keep, 2)
                os.close(keep)
            errf.seek(0)
            err = errf.read().decode(errors="replace")
        if fail is None and "prep_check: stream" in err:
            fail = "prep_check: " + err[err.index("prep_check: stream"):][:400]
        if fail:
            print(f"FAIL seed {seed} {d}: {fail}", flush=True)
            print("FAILURES 1 (stopped at the first)")
            return 1
        cov = ss.coverage(sites, hdr)
        peak = d["kind"].startswith("nrzi")
        fast = (ss.fast(st) if peak else st["redone"] == 0) and stats["exact"] == 0
        nfast += fast
        seg, n = ss.seg_counts(err)
        print(f"ok seed {seed} {d} rows {rows.shape[0]} sites {len(sites)} events {stats['events']} exact {stats['exact']} redone {st['redone']} "
              + (f"lean {st['parallel']} general {st['sequential']}" if peak else f"literal_rows {st['parallel']} from_records {st['sequential']}") + f" fast {int(fast)} | "
              + " ".join(f"{c} {cov.get(c, 0)}" for c in ss.SHAPES + (ss.PEAK_SEAMS if peak else ss.DENSE_SEAMS))
              + (" | " + " ".join(f"{k} {v // n}" for k, v in seg.items()) if n else ""), flush=True)
    print(f"FAILURES 0 ({nfast} of {ntapes} tapes on the fast paths)")
    return 0


def pe_main(make, seed0, ntapes):
    """tests/pe_util.py's check of one drawn tape per seed (P-clk: one per ladder; P-time: one per start time); the first tape that fails ends the run (no retries)"""
    import pe_shapes as ps
    import pe_util as pu
    keys = ("tracks", "sw_71_72", "sw_later", "sw_data", "sw_never", "never_past70", "marker_le70", "height_low", "near_1", "near_4", "equal")
    grand, per_cls, per_path, nev = dict.fromkeys(keys + ("f32_intervals",), 0), {}, {}, 0
    for seed in range(seed0, seed0 + ntapes):
        d = ps.draw(seed)
        for k in pu.KNOB_NAMES:
            os.environ.pop(k, None)
        os.environ.update(ps.PATHS[d["path"]])
        try:
            tapes = pu.tapes_of(d["cls"], seed, d["m"], d["invert"], d["skew"])
            pu._cache.clear()
            tot, ev = dict.fromkeys(keys + ("f32_intervals",), 0), 0
            for label, tp, att, win in tapes:
                met = ps.classes_met(tp["hdr"], att, win)
                for k, v in ps.totals(met).items():
                    if k in tot:
                        tot[k] += v
                tot["f32_intervals"] += ps.float32_intervals(met)
                stats, fe = pu.check(make, tp, att, label=label)
                ev += stats["events"]
            fail = None
        except Exception as e:                                   # a mismatch (AssertionError) or a failure of the front end
            fail = f"{type(e).__name__}: {str(e)[:2000]}"
        if fail:
            print(f"FAIL seed {seed} {d}: {fail}", flush=True)
            print("FAILURES 1 (stopped at the first)")
            return 1
        for k, v in tot.items():
            grand[k] += v
        per_cls[d["cls"]] = per_cls.get(d["cls"], 0) + 1
        per_path[d["path"]] = per_path.get(d["path"], 0) + 1
        nev += ev
        print(f"ok seed {seed} {d} tapes {len(tapes)} events {ev} | " + " ".join(f"{k} {v}" for k, v in tot.items()), flush=True)
    print("classes_met totals: " + " ".join(f"{k} {v}" for k, v in grand.items()))
    print("draws per class: " + " ".join(f"{k} {v}" for k, v in sorted(per_cls.items())) + " | per path: " + " ".join(f"{k} {v}" for k, v in sorted(per_path.items())))
    print(f"FAILURES 0 ({ntapes} draws, {nev} events compared)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
