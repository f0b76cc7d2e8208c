"""What tests/test_emul_pe_shapes.py, tests/test_gpu_pe_shapes.py and tools/fuzz_shapes.py --pe share: the committed seeds, the knob rows of the paths, the
tapes of a class with the oracle's run of each (made once a process and left unchanged), the class's counter assertion, one tape against the oracle.
Test infrastructure; the front end comes in as `make` (the emulator's or the device's)."""
import os
import tempfile

import numpy as np

import pe_shapes as ps
from parity_util import check_tape, oracle_attempts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the seeds whose counters the emulator test asserts from the oracle alone; tests/test_gpu_pe_shapes.py runs these tapes and no others
SEEDS = (0, 1)                                                         # (P-length: seed 0 has 20, 33, 34, 35 and seed 1 has 36, 37, 40, 90)
KNOB_NAMES = ("RTFE_DENSE_PATH", "RTFE_PEAK_PATH", "RTFE_GAIN_FAST", "RTFE_DS_LEAN", "RTFE_DS_WARM", "RTFE_DS_CAP", "RTFE_DENSE_DEDUP")
PATH_KNOBS = [{}, {"RTFE_DENSE_PATH": "0"}, {"RTFE_PEAK_PATH": "1"}, {"RTFE_PEAK_PATH": "1", "RTFE_GAIN_FAST": "0"}, {"RTFE_DS_LEAN": "0"}]
ids = lambda k: ",".join(f"{a[5:]}={b}" for a, b in k.items()) or "default"
TSTARTS = (0, 3_000_000_000_000)

_cache = {}
_tmp = None


def set_knobs(monkeypatch, knobs):
    for k in KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def oracle_of(tp):
    global _tmp
    if _tmp is None:
        _tmp = tempfile.TemporaryDirectory()
    wd = tempfile.mkdtemp(dir=_tmp.name)
    return oracle_attempts(tp["hdr"], tp["rows"], ps.oracle_opts(tp, wd), wd)


def tapes_of(cls, seed, m=False, invert=False, skew=False):
    """[(label, tape, the oracle's attempts, t_clkwindow per parameter set)] of class `cls`, seed `seed`: one tape, or one per clk_factor ladder (P-clk), or one
    per tstart_ns (P-time).  Computed once a process; nobody writes to what it returns."""
    key = (cls, seed, m, invert, skew)
    if key in _cache:
        return _cache[key]
    stock = lambda tp: [ps.clkwindow(tp["hdr"], p[5]) for p in ps.frontend.DEFAULT_PARMSETS[ps.frontend.PE]]
    out = []
    if cls == "P-clk":
        base = ps.tape(cls, seed, invert=invert, skew=skew)
        lad = ps.ladders(base["hdr"], oracle_of(base))
        for name in ("half", "one"):
            cfs = lad[name]
            if not m:                                                  # (without -m the reference tries the first set only - the one ON the smallest interval then; the scan still runs them all)
                cfs = [cfs[1], cfs[0]] + cfs[2:]
            tp = ps.with_ladder(base, cfs)
            if not m:
                tp = dict(tp, opts=[o for o in tp["opts"] if o != "-m"])
            out.append((name, tp, oracle_of(tp), [ps.clkwindow(tp["hdr"], c) for c in cfs]))
    elif cls == "P-time":
        for ts in TSTARTS:
            tp = ps.tape(cls, seed, invert=invert, skew=skew, m=m, tstart_ns=ts)
            out.append((f"tstart={ts}", tp, oracle_of(tp), stock(tp)))
    else:
        tp = ps.tape(cls, seed, invert=invert, skew=skew, m=m)
        out.append(("", tp, oracle_of(tp), stock(tp)))
    _cache[key] = out
    return out


def class_totals(cls, m=False, invert=False, skew=False):
    """the counters of the class's committed tapes, summed over seeds (and ladders): pe_shapes.totals plus the class's own from the sites"""
    tot = {}
    for seed in SEEDS:
        for label, tp, att, win in tapes_of(cls, seed, m, invert, skew):
            met = ps.classes_met(tp["hdr"], att, win)
            for k, v in ps.totals(met).items():
                tot[k] = min(tot.get(k, 99), v) if k == "learned_min" else tot.get(k, 0) + v
            tot["f32_intervals"] = tot.get("f32_intervals", 0) + ps.float32_intervals(met)
            tot["events"] = tot.get("events", 0) + sum(a["events"].size for a in att)
            tot["sets_tried"] = max(tot.get("sets_tried", 0), len({a["parmset"] for a in att}))
            if cls == "P-seam":
                for k, v in ps.seam_hits(tp["hdr"], met).items():
                    tot[k] = tot.get(k, 0) + v
            if cls == "P-drop":
                for place, c in ps.drop_hits(tp, att).items():
                    for k, v in c.items():
                        tot[f"{place}_{k}"] = tot.get(f"{place}_{k}", 0) + v
            if cls in ("P-shape", "P-drop"):
                tot["sites"] = tot.get("sites", 0) + len(tp["sites"])
                tot["marker_sites"] = tot.get("marker_sites", 0) + sum(bool(s.get("marker") or s.get("place") == "marker") for s in tp["sites"])
    return tot


def assert_class(cls, tot, m=True):
    """what a class's tapes must contain, from the oracle's dump: where each track switched, what it learned, and (P-seam) the cuts at the row the dump gives
    the marker peak.  Where a shape or a dropout was written only the generator knows (`sites`, `marker_sites`); P-drop looks up, per site, what the dump
    says of that attempt and track (pe_shapes.drop_hits).  The bounds are counts of tracks: 9 = every track of one block."""
    need = {
        # 36: the switch at peak 72; 37, 40, 90: later, at the marker; 20, 33, 34, 35: the marker at 70 or less and the switch inside the data
        "P-length": dict(sw_71_72=9, sw_later=27, sw_data=27, marker_le70=36),
        # a mark of 72 or 90 flux changes: six tracks whose count passes 70 and that never switch; the blocks' tracks switch
        "P-mark": dict(never_past70=12, sw_71_72=9, sw_later=9),
        # the count lags behind the marker; nobody reaches the switch without a height; every track with a dropout over peaks 4 .. 16 learned a small
        # height or full-size peaks behind a lagging count (learn_miss == 0 below), some of each; the dropouts over 60 .. 76 made the count lag
        "P-drop": dict(marker_le70=6, sw_data=6, height_low=2, learned_small=2, learned_min=1, marker_sites=4, learn_n=6, learn_small=2, learn_lag=3, count_lag=8, marker_moved=3),
        # candidates within one half sample of a window (they are one float32 either side of it), switches on both sides, every set tried
        "P-clk": dict(near_1=100, sw_71_72=20, sw_later=20, sw_data=20),
        "P-jit": dict(near_1=9, near_4=50, sw_data=9),
        "P-shape": dict(sites=80, marker_sites=40, sw_71_72=5, sw_later=20),
        "P-seam": dict(dseg_sub=18, dseg_tile=9, dseg_warm=9, sw_71_72=18, sw_later=27),
        "P-time": dict(sw_71_72=18, sw_later=54, sw_data=54),
    }[cls]
    if cls == "P-clk" and not m:                                      # (the reference then tries the first set only: the window under the smallest half-bit interval)
        need = dict(near_1=20, sw_71_72=9, equal=1)
    for k, v in need.items():
        assert tot.get(k, 0) >= v, (cls, k, v, tot)
    if cls == "P-drop":
        assert tot["learn_miss"] == 0, tot
    assert tot["events"] > 5000, tot


def check(make, tp, att, scans=2, label=""):
    """one tape against the oracle, every event field, `scans` scans of one fresh handle; returns (check_tape's stats, the handle)"""
    fe = make(ps.config(tp))
    for rep in range(scans):
        msgs, stats = check_tape(fe, tp["hdr"], tp["rows"], att)
        assert not msgs, f"{tp['cls']} seed {tp['seed']} {label} {' '.join(tp['opts'])} scan {rep}: " + "\n".join(msgs[:8])
        assert stats["events"] > 0 and stats["speculative"] + stats["exact"] == len(att), (stats, len(att))
    return stats, fe


def check_class(make, cls, m=False, invert=False, skew=False):
    """every committed tape of the class against the oracle; returns the events compared"""
    n = 0
    for seed in SEEDS:
        for label, tp, att, win in tapes_of(cls, seed, m, invert, skew):
            stats, fe = check(make, tp, att, label=label)
            n += stats["events"]
    return n


def same_results(make, cfg, rows, monkeypatch, variants):
    """one scan per knob set: the same counts, the same published fields of the burst table and, per (burst, parameter set, track), the same events byte for byte"""
    out = []
    for knobs in variants:
        set_knobs(monkeypatch, knobs)
        out.append(make(cfg).scan(rows).fetch())
    r0 = out[0]
    assert r0.nbursts > 0 and int(np.asarray(r0.counts).sum()) > 1000
    # RTFE_F_SCREEN_UNDERFLOW belongs to the paths that screen candidates (k_decode, the peak path): a threshold fell below the screen and the burst wants an exact
    # rescan - P-drop's small heights bring that.  The dense path screens nothing and never sets it; a burst a path has flagged so promises no events
    under = ps.frontend.F_SCREEN_UNDERFLOW
    assert not (r0.bursts["flags"][:r0.nbursts] & under).any()
    for knobs, r in zip(variants[1:], out[1:]):
        assert r.nbursts == r0.nbursts, knobs
        for k in ("zone_first", "zone_end", "reset_sample", "safe_last", "end_sample"):
            assert (r.bursts[k][:r.nbursts] == r0.bursts[k][:r0.nbursts]).all(), (knobs, k)
        assert ((r.bursts["flags"][:r.nbursts] & ~np.uint32(under)) == r0.bursts["flags"][:r0.nbursts]).all(), (knobs, "flags")
        skipped = int(((r.bursts["flags"][:r.nbursts] & under) != 0).sum())
        assert 2 * skipped < r0.nbursts, (knobs, f"{skipped} of {r0.nbursts} bursts want a rescan: most must be compared byte for byte")
        for b in range(r0.nbursts):
            if int(r.bursts["flags"][b]) & under:
                continue
            for p in range(len(cfg.parmsets)):
                for t in range(cfg.ntrks):
                    assert r.track_events(b, p, t).tobytes() == r0.track_events(b, p, t).tobytes(), (knobs, b, p, t)
    return r0


def preamble_cut(tp, peak=66, block=1):
    """(the tape with quiet rows in front so that a multiple of 1024 lies on peak `peak` of the preamble of block `block`, that row)"""
    b = tp["meta"][block]
    r = ps.peak_row(tp["rows"], tp["spb"], b, 0, peak)
    k = -r % 1024
    rows = np.ascontiguousarray(np.concatenate([np.zeros((k, tp["rows"].shape[1]), tp["rows"].dtype), tp["rows"]]))
    assert (r + k) % 1024 == 0 and peak < ps.marker_peak(b)
    return rows, r + k


def fragments_case(make, tp, peak=66):
    """the tape as two fragments cut inside a preamble (own_rows): the first owns the bursts that begin in front of the cut and reads on behind it, the second
    starts in the middle of the preamble.  Together the whole-tape scan's bursts and events."""
    from readtape_amd import shard
    rows, cut = preamble_cut(tp, peak)
    fe = make(ps.config(tp))
    whole = fe.scan(rows).fetch()
    wb = shard.absolute_bursts(whole, 0)
    we = shard.flatten_events(whole, wb, 0)
    key = lambda e: e[np.lexsort((e[:, 1], e[:, 0]))]
    assert any(int(a) < cut < int(z) for a, z in zip(wb["reset_sample"], wb["end_sample"])), "the cut lies in no burst"
    nb, fl, ev = 0, [], []
    bounds = [0, cut, rows.shape[0]]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        r = fe.scan(np.ascontiguousarray(rows[lo:]), row_base=lo, first_is_tape_start=lo == 0, own_rows=hi - lo).fetch()
        b = shard.absolute_bursts(r, lo)
        nb += r.nbursts; fl.append(b["flags"]); ev.append(shard.flatten_events(r, b, 0))
    assert nb == whole.nbursts, (cut, nb, whole.nbursts)
    assert not ((np.concatenate(fl) & ~np.uint32(1)).any()), cut
    got = np.concatenate(ev)
    assert got.shape == we.shape and (key(got) == key(we)).all(), cut
    return we.shape[0]
