"""GPU box: what a -zeros -differentiate scan costs with k_diffz, against another build of the front end (the commit in front of it: k_decode's
walk_diffzeros, a lane per track) - whole scans of a resident 9-track GCR tape, timed with HIP events.

  python tools/gpu_diffz_time.py --other PATH/librtfe.so [--rows 1e8] [--base-rows 5e6] [--repeats 4] [--rounds 2]

The two libraries take turns, a fresh child process each (RTFE_LIB_PATH picks the library; a process never replaces its own program): `rounds` x
(other, this build), every child two warm-up scans and `repeats` timed ones on the same tape.  The first child of each library also fetches the scan:
counts and a digest of the burst table's fields and of every event list.  Nothing is printed about time unless both agree byte for byte.  Then, per
library, median and min - max of all its timed scans; the condition this build is held to is  median(this) < min(other).  For context the same rows with
plain -zeros (k_zeros), this build, and the spans rtfe_kernel_ms reports (k_diffz is timed in the k_zeros span).
A child: python tools/gpu_diffz_time.py --child BASE.npz ... (not for the command line)."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    import numpy as np
    import torch
    from readtape_amd import frontend, tbin
    z = np.load(a.child, allow_pickle=True)
    hdr = tbin.TbinHeader(**json.loads(str(z["hdr"])))
    base = z["rows"]
    k = max(1, int(a.rows // base.shape[0]))
    rows = torch.from_numpy(base).cuda().repeat(k, 1).contiguous()
    out = {"lib": os.environ.get("RTFE_LIB_PATH", "this build"), "rows": int(rows.shape[0])}
    for name, kw in (("diffz", {"find_zeros": True, "differentiate": True}),) + ((("zeros", {"find_zeros": True}),) if a.zeros else ()):
        fe = frontend.FrontEnd(frontend.FrontEndConfig.from_header(hdr, nparmsets=1, **kw))
        if hasattr(fe.lib, "rtfe_detector_path"):
            out[name + "_path"] = fe.detector_path
        for _ in range(2):
            r = fe.scan(rows)
            torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fe.scan(rows)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        out[name + "_ms"] = ms
        fe.set_timing(True)
        fe.scan(rows)
        spans, n = fe.kernel_ms()
        fe.set_timing(False)
        out[name + "_spans"] = {s: round(v / max(n, 1), 3) for s, v in spans.items() if v > 0.001}
        if name == "diffz":
            r = fe.scan(rows).fetch(events=a.digest)
            out["bursts"] = int(r.nbursts)
            out["events"] = int(r.counts.sum())
            if a.digest:
                h = hashlib.sha256()
                h.update(r.counts.tobytes())
                for f in ("zone_first", "zone_end", "reset_sample", "safe_last", "end_sample", "flags"):
                    h.update(np.ascontiguousarray(r.bursts[f]).tobytes())
                for b in range(r.nbursts):
                    for t in range(hdr.ntrks):
                        h.update(r.track_events(b, 0, t).tobytes())
                out["digest"] = h.hexdigest()
        del fe, r
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other")
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--base-rows", type=float, default=5e6)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child")
    ap.add_argument("--digest", action="store_true")
    ap.add_argument("--zeros", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    assert a.other and os.path.exists(a.other), "--other: the library to compare against"
    assert a.repeats * a.rounds >= 7, "at least seven timed scans a library"
    import dataclasses
    import numpy as np
    import bench
    base = bench.make_base_tape(seed=1003, target_rows=a.base_rows, kind="gcr")
    hdr = base.spec.header()
    res = {"other": [], "this": []}
    with tempfile.TemporaryDirectory() as wd:
        path = os.path.join(wd, "base.npz")
        np.savez(path, rows=base.rows, hdr=json.dumps(dataclasses.asdict(hdr)))
        del base
        for rnd in range(a.rounds):
            for who in ("other", "this"):
                env = dict(os.environ)
                env.pop("RTFE_LIB_PATH", None)
                env.pop("RTFE_DIFFZ_KERNEL", None)
                if who == "other":
                    env["RTFE_LIB_PATH"] = os.path.abspath(a.other)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", path, "--rows", str(a.rows), "--repeats", str(a.repeats)]
                cmd += (["--digest"] if rnd == 0 else []) + (["--zeros"] if who == "this" and rnd == 0 else [])
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
                line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
                if p.returncode != 0 or line is None:       # (nothing more is started on the device behind a child that failed)
                    print(p.stdout[-2000:], p.stderr[-4000:], sep="\n")
                    print(f"child ({who}, round {rnd}) failed: exit status {p.returncode}")
                    return 1
                res[who].append(json.loads(line[7:]))
    o0, t0 = res["other"][0], res["this"][0]
    same = all(o0[k] == t0[k] for k in ("rows", "bursts", "events", "digest"))
    print(f"rows {t0['rows']} bursts {t0['bursts']} events {t0['events']}  counts, burst fields and event bytes {'identical' if same else 'DIFFER'}: {o0['digest'][:16]} / {t0['digest'][:16]}")
    if not same:
        return 1
    stat = {}
    for who in ("other", "this"):
        ms = [x for r in res[who] for x in r["diffz_ms"]]
        stat[who] = (statistics.median(ms), min(ms), max(ms), len(ms))
        print(f"{who:5s} -zeros -differentiate: median {stat[who][0]:.3f} ms  min {stat[who][1]:.3f}  max {stat[who][2]:.3f}  ({stat[who][3]} scans; path {res[who][0].get('diffz_path', 'n/a')}; "
              f"spans {res[who][0]['diffz_spans']})")
    zms = t0.get("zeros_ms", [])
    if zms:
        print(f"this  -zeros (context, {t0.get('zeros_path')}): median {statistics.median(zms):.3f} ms  min {min(zms):.3f}  max {max(zms):.3f}  (spans {t0['zeros_spans']})")
    kms = t0["diffz_spans"].get("k_zeros", 0.0)
    nbytes = t0["rows"] * 2 * hdr.ntrks + 16 * t0["events"]
    if kms > 0:
        print(f"k_diffz {kms:.3f} ms; algorithmic bytes (rows once + 16 B an event) {nbytes / 1e9:.3f} GB -> {nbytes / kms / 1e6:.1f} GB/s = {100 * nbytes / kms / 1e6 / 8000:.1f} % of 8 TB/s")
    ok = stat["this"][0] < stat["other"][1]
    print(f"median(this) {stat['this'][0]:.3f} ms {'<' if ok else '>='} min(other) {stat['other'][1]:.3f} ms: {'condition met' if ok else 'CONDITION NOT MET'}; ratio of medians {stat['other'][0] / stat['this'][0]:.2f}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
