"""What tests/test_emul_seam_shapes.py, tests/test_gpu_seam_shapes.py and tools/fuzz_shapes.py --seams share: the knob rows and seeds, one shaped tape against
the oracle (seam_tape), the rows of one format under one knob row with their coverage (peak_rows, dense_rows), a phase, path against path, fragments.
Test infrastructure; the front end comes in as `make` (the emulator's or the device's)."""
import os

import numpy as np

import seam_shapes as ss
from parity_util import check_tape, config_for, oracle_attempts
from readtape_amd import shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOB_NAMES = ("RTFE_SEG_RECS", "RTFE_SEG_WARM", "RTFE_SEG_REJOIN", "RTFE_PREP_RUN", "RTFE_GAIN_FAST", "RTFE_SIFT_GENERIC", "RTFE_SIFT_PLAIN", "RTFE_PK_MAR", "RTFE_PEAK_PATH",
              "RTFE_DENSE_PATH", "RTFE_DS_WARM", "RTFE_DS_CAP")
PEAK_KNOBS = [{}, {"RTFE_SEG_RECS": "32"}, {"RTFE_SEG_RECS": "32", "RTFE_SEG_WARM": "3"}, {"RTFE_SEG_RECS": "32", "RTFE_SEG_WARM": "3", "RTFE_SEG_REJOIN": "0"}, {"RTFE_PREP_RUN": "2"}]
PATH_KNOBS = [{"RTFE_GAIN_FAST": "0"}, {"RTFE_SIFT_GENERIC": "1"}, {"RTFE_PK_MAR": "0"}, {"RTFE_PEAK_PATH": "0"}]
DENSE_KNOBS = [{}, {"RTFE_DS_WARM": "8"}, {"RTFE_DS_CAP": "3"}]
# the seeds whose coverage is asserted here; tests/test_gpu_seam_shapes.py runs these tapes and no others
PEAK_SEEDS = {"nrzi9": (1, 2), "nrzi7": (3, 4), "nrzi9_m": (1, 2)}
DENSE_SEEDS = {"gcr": (5, 6), "gcr_m": (5, 6), "pe": (5, 6)}
PHASE_SEEDS = {"nrzi9": 2, "nrzi7": 3}
MIN_SHAPES, MIN_SEAMS = 5, 3                                           # (the thresholds of tests/test_emul_zeros_shapes.py)
ids = lambda k: ",".join(f"{a[5:]}={b}" for a, b in k.items()) or "default"


def set_knobs(monkeypatch, knobs):
    for k in KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def seam_tape(make, hdr, rows, opts, wd, scans=2):
    """one tape against the oracle, every event field, `scans` scans of one fresh handle (the second runs under the floor the first one learned).  Returns
    (check_tape's stats, the last scan's stats, did the fast paths take it: nothing redone, no chain gave up, no exact rescan, lean > 2 x general)."""
    os.makedirs(wd, exist_ok=True)
    att = oracle_attempts(hdr, rows, opts, wd)
    fe = make(config_for(hdr, opts))
    for rep in range(scans):
        msgs, stats = check_tape(fe, hdr, rows, att)
        assert not msgs, f"scan {rep}: " + "\n".join(msgs[:8])
        assert stats["events"] > 0 and stats["speculative"] + stats["exact"] == len(att), (stats, len(att))
    st = fe.scan_stats(fe.scan(rows).fetch())
    return stats, st, att


def add(cov, more):
    for k, v in more.items():
        cov[k] = cov.get(k, 0) + v


def peak_rows(make, kind, knobs, wd, capfd=None):
    """the seeds of one format under one knob row: every tape against the oracle; returns (coverage of the tapes that qualify, their seg_shapes: counts, how many
    qualified)"""
    cov, seg, nq = {}, dict.fromkeys(ss.SEG_COUNTS, 0), 0
    for seed in PEAK_SEEDS[kind]:
        hdr, rows0, rows, sites, opts = ss.shaped(seed, kind=kind)
        if capfd is not None:
            capfd.readouterr()
        stats, st, att = seam_tape(make, hdr, rows, opts, os.path.join(wd, str(seed)))
        err = capfd.readouterr().err if capfd is not None else ""
        assert "prep_check: stream" not in err, err[:2000]               # (what kCrClear promises, checked on the finished streams)
        print(kind, seed, ids(knobs), stats, {k: st[k] for k in ("redone", "parallel", "sequential", "gave_up")})
        if not (ss.fast(st) and stats["exact"] == 0):
            continue
        nq += 1
        add(cov, ss.coverage(sites, hdr, prep_run=int(knobs.get("RTFE_PREP_RUN", ss.PREP_RUN))))
        tot, n = ss.seg_counts(err)
        if capfd is not None:
            assert n >= 3, "no seg_shapes: line"
            add(seg, {k: v // n for k, v in tot.items()})                # (per scan)
    return cov, seg, nq


PHASES = [("nrzi9", k) for k in range(14)] + [("nrzi7", k) for k in range(14)] + [("nrzi9", k) for k in (14, 15, 16, 17)]


def phase_case(make, kind, k, wd):
    """a shaped tape behind k quiet rows: the shapes as they were, every row grid moved by k - against the oracle's run of the same rows"""
    hdr, rows0, rows, sites, opts = ss.shaped(PHASE_SEEDS[kind], kind=kind)
    rows = ss.phased(rows, k)
    stats, st, att = seam_tape(make, hdr, rows, opts, wd, scans=1)
    assert ss.fast(st) and stats["exact"] == 0, (stats, st)
    return ss.coverage(ss.phase_sites(sites, k), hdr)


def same_results(make, cfg, rows, monkeypatch, variants):
    """one scan per knob set: the same counts, the same published fields of the burst table and, per (burst, parameter set, track), the same events byte for byte"""
    out = []
    for knobs in variants:
        set_knobs(monkeypatch, knobs)
        out.append(make(cfg).scan(rows).fetch())
    r0 = out[0]
    assert r0.nbursts > 0 and int(r0.counts.sum()) > 100
    for knobs, r in zip(variants[1:], out[1:]):
        assert r.nbursts == r0.nbursts and (np.asarray(r.counts) == np.asarray(r0.counts)).all(), knobs
        for k in ("zone_first", "zone_end", "reset_sample", "safe_last", "end_sample", "flags"):
            assert (r.bursts[k][:r.nbursts] == r0.bursts[k][:r0.nbursts]).all(), (knobs, k)
        for b in range(r0.nbursts):
            for p in range(len(cfg.parmsets)):
                for t in range(cfg.ntrks):
                    assert r.track_events(b, p, t).tobytes() == r0.track_events(b, p, t).tobytes(), (knobs, b, p, t)
    return r0


def dense_rows(make, kind, knobs, wd):
    """the seeds of one dense format under one knob row against the oracle; returns (coverage, rows k_dchain walked literally, events it made from records,
    the events they are a share of, how many tapes qualified) over the tapes that qualify: nothing redone, no exact rescan.  The events: the oracle's; under -m
    the scan's own, counted - as the events from records then are - with every parameter set a chain of its own (a second handle under RTFE_DENSE_DEDUP=0)."""
    cov, lit, rec, ev, nq = {}, 0, 0, 0, 0
    warm = int(knobs["RTFE_DS_WARM"]) if "RTFE_DS_WARM" in knobs else None
    for seed in DENSE_SEEDS[kind]:
        hdr, rows0, rows, sites, opts = ss.shaped(seed, kind=kind)
        stats, st, att = seam_tape(make, hdr, rows, opts, os.path.join(wd, str(seed)))
        print(kind, seed, ids(knobs), stats, {k: st[k] for k in ("redone", "parallel", "sequential", "gave_up")})
        if st["redone"] or stats["exact"]:
            continue
        nq += 1
        add(cov, ss.coverage(sites, hdr, warm=warm))
        n_rec, n_ev = st["sequential"], stats["events"]
        if "-m" in opts:
            old = os.environ.get("RTFE_DENSE_DEDUP")
            os.environ["RTFE_DENSE_DEDUP"] = "0"
            try:
                fe = make(config_for(hdr, opts))
                res = fe.scan(rows).fetch()
                n_rec, n_ev = fe.scan_stats(res)["sequential"], int(np.asarray(res.counts).sum())
            finally:
                if old is None:
                    del os.environ["RTFE_DENSE_DEDUP"]
                else:
                    os.environ["RTFE_DENSE_DEDUP"] = old
        lit, rec, ev = lit + st["parallel"], rec + n_rec, ev + n_ev
    return cov, lit, rec, ev, nq


def fragment_cuts(sites, lo, hi, n=2):
    """multiples of 1024 (the grid shard.py and ingest.py cut on) inside rows [lo, hi) that a site straddles"""
    cuts = sorted({c for s in sites for c in range(s["lo"] + 1, s["hi"] + 1) if c % 1024 == 0 and lo <= c < hi})
    return cuts[len(cuts) // 3:: max(1, len(cuts) // n)][:n]


def fragments_case(make, kind, seed):
    """the tape as three fragments: the first ends in the gap in front of the longest block behind the first, at a multiple of 1024 that is none of 896 - the second decodes that
    block on row grids of its own; it ends at a multiple of 1024 inside the block where a shape lies across the cut (its halo reaches on), and the third starts
    there in the middle of the data.  Together the whole-tape scan's bursts and events."""
    hdr, rows0, rows, sites, opts = ss.shaped(seed, kind=kind)
    fe = make(config_for(hdr, opts))
    whole = fe.scan(rows).fetch()
    wb = shard.absolute_bursts(whole, 0)
    we = shard.flatten_events(whole, wb, 0)
    key = lambda e: e[np.lexsort((e[:, 1], e[:, 0]))]
    big = 1 + int(np.argmax((wb["end_sample"].astype(np.int64) - wb["reset_sample"].astype(np.int64))[1:]))      # (the longest block behind the first)
    a = (int(wb["zone_first"][big]) // 1024 + 1) * 1024
    assert a % ss.K_SF_TILE and a + 1024 < int(wb["zone_end"][big]), (a, wb[big])
    cuts = fragment_cuts(sites, int(wb["reset_sample"][big]) + 1024, int(wb["end_sample"][big]) - 1024)
    assert len(cuts) >= 2, cuts
    for cut in cuts:
        bounds = [0, a, cut, rows.shape[0]]
        nb, fl, ev = 0, [], []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            r = fe.scan(np.ascontiguousarray(rows[lo:]), row_base=lo, first_is_tape_start=lo == 0, own_rows=hi - lo).fetch()
            b = shard.absolute_bursts(r, lo)
            nb += r.nbursts; fl.append(b["flags"]); ev.append(shard.flatten_events(r, b, 0))
        assert nb == whole.nbursts, (cut, nb, whole.nbursts)
        assert not ((np.concatenate(fl) & ~np.uint32(1)).any()), cut
        got = np.concatenate(ev)
        assert got.shape == we.shape and (key(got) == key(we)).all(), cut
