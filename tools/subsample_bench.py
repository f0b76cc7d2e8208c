"""-subsample on the device, measured (profiles/subsample_stream.txt is this tool's output on an MI355X).

1. The kernel alone.  rtfe_decimate_rows on a raw window of the shape the streaming reader's defaults produce (window_rows 2^24 + halo_rows 2^17 used
   rows, nine tracks, subsample 2 and 4) against what the code before it would have to run for the same result: the strided tensor copy
   pipeline.decode_tape uses, plus rtfe_find_end_mark over the raw rows.  Device events around every call, a warm-up, the candidates alternating in
   one process (yardstick, new, yardstick), enough rounds for `--seconds` of device time per candidate.  The two yardstick series say what the
   run-to-run spread is; the gate is  median(new) <= median(yardstick) + spread.
   The rate is (raw bytes + kept bytes) / time - every raw byte is read once, every kept byte written once - and is given as a share of the HBM peak
   (8.0 TB/s by the data sheet, 6.29 TB/s for a measured float4 copy).
2. End to end, for information (--e2e): a tape streamed from a file as it is, and the same tape with every row written twice streamed with
   subsample=2 - the same used rows, so the same .tap - through ingest.decode_file_streaming.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def kernel_alone(torch, used_rows, ntrks, n, seconds, say):
    from readtape_amd import frontend, synth
    lib, be = frontend._load_library(), frontend.TorchBackend()
    fe = frontend.FrontEnd(frontend.FrontEndConfig.from_header(synth.nrzi_spec(ntrks=ntrks).header()))      # (rtfe_find_end_mark wants a handle)
    raw = torch.randint(-32767, 32768, (used_rows * n, ntrks), dtype=torch.int16, device="cuda")
    out_new, out_old = (torch.empty((used_rows, ntrks), dtype=torch.int16, device="cuda") for _ in range(2))
    m_new, m_old = be.empty(16), be.empty(16)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream

    def new():
        frontend.decimate_rows(lib, be, raw, used_rows * n, n - 1, n, out_new, m_new, st)

    def old():
        out_old.copy_(raw[n - 1::n])
        if lib.rtfe_find_end_mark(fe.h, raw.data_ptr(), used_rows * n, m_old.data_ptr(), st) != 0:
            raise RuntimeError(lib.rtfe_last_error().decode())

    def timed(fn, reps):
        evs = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream); fn(); b.record(stream)
            evs.append((a, b))
        return evs

    for fn in (old, new, old, new):                       # warm-up
        fn()
    torch.cuda.synchronize()
    assert torch.equal(out_new, out_old) and torch.equal(m_new[:8], m_old[:8])
    probe = timed(old, 3) + timed(new, 3)
    torch.cuda.synchronize()
    per_round = sum(a.elapsed_time(b) for a, b in probe) / 3 / 1e3
    rounds = max(20, int(2 * seconds / max(per_round, 1e-6)))
    series = {"yardstick_a": [], "new": [], "yardstick_b": []}
    for _ in range(rounds):                               # yardstick, new, yardstick - alternating
        series["yardstick_a"] += timed(old, 1)
        series["new"] += timed(new, 1)
        series["yardstick_b"] += timed(old, 1)
    torch.cuda.synchronize()
    ms = {k: sorted(a.elapsed_time(b) for a, b in v) for k, v in series.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    q = lambda v, f: v[min(len(v) - 1, int(f * len(v)))]
    yard = (med["yardstick_a"] + med["yardstick_b"]) / 2
    both = sorted(ms["yardstick_a"] + ms["yardstick_b"])
    spread = max(abs(med["yardstick_a"] - med["yardstick_b"]), (q(both, 0.75) - q(both, 0.25)) / 2)
    nbytes = (used_rows * n + used_rows) * 2 * ntrks
    rate = nbytes / (med["new"] / 1e3)
    res = dict(subsample=n, ntrks=ntrks, used_rows=used_rows, raw_mb=round(used_rows * n * 2 * ntrks / 1e6, 1), rounds=rounds,
               new_ms=round(med["new"], 4), new_ms_p25_p75=[round(q(ms["new"], 0.25), 4), round(q(ms["new"], 0.75), 4)],
               yardstick_ms=round(yard, 4), yardstick_a_ms=round(med["yardstick_a"], 4), yardstick_b_ms=round(med["yardstick_b"], 4), spread_ms=round(spread, 4),
               new_tb_per_s=round(rate / 1e12, 3), share_of_hbm_spec=round(rate / HBM_SPEC, 3), share_of_measured_copy=round(rate / HBM_COPY, 3),
               yardstick_tb_per_s_same_bytes=round(nbytes / (yard / 1e3) / 1e12, 3), gate_new_not_slower=bool(med["new"] <= yard + spread))
    say(json.dumps(res))
    fe.close()
    return res


def end_to_end(torch, say, target_rows, copies):
    import bench
    from readtape_amd import ingest, pipeline, tbin
    tape = bench.make_base_tape(seed=1000, target_rows=target_rows, kind="nrzi")
    hdr = tape.spec.header()
    rows = np.tile(tape.rows, (copies, 1))
    opts = pipeline.DecodeOptions(verbose=False)
    kw = dict(window_rows=1 << 22, halo_rows=1 << 18, opts=opts, replay_threads=16, read_threads=8, replay_split=8)
    with tempfile.TemporaryDirectory() as wd:
        a, b = os.path.join(wd, "a.tbin"), os.path.join(wd, "b.tbin")
        tbin.write_tbin(a, hdr, rows)
        tbin.write_tbin(b, hdr, np.repeat(rows, 2, axis=0))      # every row twice: subsample=2 uses the same rows
        del rows
        out = {}
        for name, path, extra in (("as_it_is", a, {}), ("oversampled_subsample_2", b, dict(subsample=2))):
            ingest.decode_file_streaming(path, os.path.join(wd, "w.tap"), **kw, **extra)      # untimed pass, as bench.py's e2e line has
            os.sync()
            runs = [ingest.decode_file_streaming(path, os.path.join(wd, name + ".tap"), **kw, **extra) for _ in range(3)]
            best = max(runs, key=lambda s: s["msamples_per_s"])
            out[name] = dict(used_msamples_per_s=[round(s["msamples_per_s"], 1) for s in runs], rows=best["rows"], raw_rows=best["raw_rows"], windows=best["windows"],
                             seconds=round(best["seconds"], 4), blocks=best["blocks"])
        out["tap_identical"] = open(os.path.join(wd, "as_it_is.tap"), "rb").read() == open(os.path.join(wd, "oversampled_subsample_2.tap"), "rb").read()
    say(json.dumps({"e2e_for_information": out}))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--subsample", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--used-rows", type=int, default=(1 << 24) + (1 << 17), help="rows of the thinned window (the streaming defaults: window_rows + halo_rows)")
    ap.add_argument("--ntrks", type=int, default=9)
    ap.add_argument("--seconds", type=float, default=0.5, help="device time per candidate")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--e2e-rows", type=float, default=5e6)
    ap.add_argument("--e2e-copies", type=int, default=8)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"

    def say(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    say(json.dumps(dict(tool="tools/subsample_bench.py", device=torch.cuda.get_device_name(0), hbm_spec_tb_per_s=HBM_SPEC / 1e12, hbm_measured_copy_tb_per_s=HBM_COPY / 1e12)))
    ok = True
    for n in args.subsample:
        ok &= kernel_alone(torch, args.used_rows, args.ntrks, n, args.seconds, say)["gate_new_not_slower"]
    if args.e2e:
        end_to_end(torch, say, args.e2e_rows, args.e2e_copies)
    say(json.dumps(dict(kernel_gate_met=bool(ok))))


if __name__ == "__main__":
    main()
