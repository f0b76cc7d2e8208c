"""-zeros -differentiate: the seams of k_diffz (rtfe_diffz.hip), the shapes that decide its three-state transducer written on them, and the cases
tests/test_emul_diffz_kernel.py and tests/test_gpu_diffz_kernel.py share.  Test infrastructure.

k_diffz cuts a burst's rows [restart, stop) into a literal head of KDZ_HEAD rows and sub-segments of KDZ_SUB rows (the last one may be shorter), which it
takes in chunks of KDZ_THREADS // ntrks: a sub-segment's map from "none" (pass 1), the composition of a chunk's maps in order, the events (pass 2).  What
can go wrong lies where a pending crossing, its first / last exact zero or an event slot is handed from one sub-segment, chunk or the head to the next.
zeros_shapes.shape_rows(diff=True) writes D-run / D-band / D-skip and the zero shapes; this module adds, on k_diffz's seams and at random places,
  D-long   arm, then 130 .. 400 flat raw rows (exact zeros after the differentiator, across two and more sub-segments, d1 below and above 255), confirm
  D-rearm  a second |v| > 0.2 of the same sign while the crossing is pending, exact zeros in front of it and behind it (t_firstzero starts again)
  D-small  a confirmation by a sample inside (0, 0.2] - which must not arm the other direction: the same small step back follows and must stay silent.
           Such a sample exists only where samples_per_bit < 10 (the dead band is 0.05 V, the scale 0.4 x samples_per_bit): tapes of odd seeds carry
           twice the speed in their header (the oracle reads the same header; what the block decoders make of it is compared like everything else).
Every site records the rows it spans, so that coverage() counts the seams a shape lies ACROSS, against the burst table of the shaped tape's own scan."""
import dataclasses
import os
import re

import numpy as np

import emul_util
import zeros_shapes as zs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIFFZ_SRC = os.path.join(ROOT, "readtape_amd", "csrc", "rtfe_diffz.hip")

# the seams, mirrored from the kernel (kernel_constants() reads them from the source)
KDZ_HEAD, KDZ_SUB, KDZ_THREADS = 64, 128, 256
NEW_SHAPES = ("D-long", "D-rearm", "D-small")
SEAMS = ("dz_head", "dz_sub", "dz_chunk", "dz_last")
MIN_SEAMS = 3
KNOB = "RTFE_DIFFZ_KERNEL"


def chunk_subs(ntrks):
    """sub-segments k_diffz takes in one pass: a lane per (sub-segment, track)"""
    return KDZ_THREADS // ntrks


def kernel_constants(root=ROOT):
    """(kDzHead, kDzSub, kDzThreads, the chunk expression) as rtfe_diffz.hip has them"""
    s = open(os.path.join(root, "readtape_amd", "csrc", "rtfe_diffz.hip")).read()
    num = lambda name: int(re.search(r"\b" + name + r"\s*=\s*(\d+)", s).group(1))
    chunk = re.search(r"const int nsub_max = (kDzThreads / ntrks);", s)
    return num("kDzHead"), num("kDzSub"), num("kDzThreads"), chunk.group(1) if chunk else None


def build_emul():
    """emul_util.build_emul() does not know rtfe_diffz.hip: the library is built again where that file is newer"""
    so = emul_util.EMUL_SO
    if os.path.exists(so) and os.path.getmtime(DIFFZ_SRC) > os.path.getmtime(so):
        try:
            os.remove(so)
        except FileNotFoundError:
            pass
    return emul_util.build_emul()


def emul_frontend(cfg, tile_rows=512):
    build_emul()
    return emul_util.emul_frontend(cfg, tile_rows=tile_rows)


def spb_of(hdr):
    return int(1 / (np.float32(hdr.bpi) * np.float32(hdr.ips) * np.float32(hdr.tdelta_ns * 1e-9)))


def diff_v(raw, prev, mv, spb):
    """differentiate() for one sample in float, as the reference and the kernels compute it (src/readtape.c:1383-1388)"""
    d = zs.volt(raw, mv) - zs.volt(prev, mv)
    if d < np.float32(0.05) and d > np.float32(-0.05):
        d = np.float32(0)
    return np.float32(np.float32(d * np.float32(0.4)) * np.float32(spb))


def seam_rows(spans, ntrks):
    """{seam class: rows} of a scan's burst spans: the first row behind the head, the first rows of the sub-segments, those that begin a chunk, and the
    first row of a burst's last sub-segment where that one is shorter than the others"""
    out = {s: [] for s in SEAMS}
    for reset, end in spans:
        c0 = reset + KDZ_HEAD
        if end > c0 - 2:
            out["dz_head"].append(c0)
        nsub = max(0, -(-(end - c0) // KDZ_SUB))
        for j in range(1, nsub):
            out["dz_chunk" if j % chunk_subs(ntrks) == 0 else "dz_sub"].append(c0 + j * KDZ_SUB)
        if nsub >= 1 and (end - c0) % KDZ_SUB:
            out["dz_last"].append(c0 + (nsub - 1) * KDZ_SUB)
    return out


def seams_of(lo, hi, ntrks, spans):
    """the seam classes a shape that spans rows [lo, hi] lies across: the seam's row and the row in front of it both inside the shape"""
    return {s for s, at in seam_rows(spans, ntrks).items() if any(lo <= r - 1 and r <= hi for r in at)}


def coverage(sites, hdr, nrows, bursts):
    """{class: count}: shape classes as written, k_diffz's seam classes recomputed against `bursts` (zeros_shapes' sites span their row +- 2)"""
    cnt = {}
    spans = zs.burst_spans(bursts, nrows, zs.tail_rows(hdr))
    for s in sites:
        cnt[s["shape"]] = cnt.get(s["shape"], 0) + 1
        for sm in seams_of(s.get("lo", s["row"] - 2), s.get("hi", s["row"] + 2), hdr.ntrks, spans):
            cnt[sm] = cnt.get(sm, 0) + 1
    return cnt


def add_shapes(hdr, rows0, rows_in, sites_in, bursts, rng, per_seam=2, nrandom=6):
    """rows_in (zeros_shapes' shaped rows of rows0) with the new classes on k_diffz's seams - as `bursts`, a -zeros -differentiate scan's table, has
    them - and at `nrandom` random places a class.  Returns (rows, sites_in + the new sites)."""
    rows = rows_in.astype(np.int64).copy()
    nrows, ntrks = rows.shape
    mv = hdr.maxvolts
    spb = max(1, spb_of(hdr))
    busy = np.zeros((nrows, ntrks), bool)                       # the new sites' rows
    spbm = max(spb, 19)

    def extent(s):                                               # (zeros_shapes' own shapes: a sub-segment and a half for the long ones, else two bit cells)
        return s["row"] - 2 * spbm - 8, s["row"] + (2 * zs.KZP_SUB + 80 if s["shape"] in ("Z-slow", "Z-sub") else 3 * spbm + 16)
    old = [dict(s, ext=extent(s)) for s in sites_in]            # a new shape may be written over them: such a site is dropped from the list
    sites = []
    peak = np.abs(rows0.astype(np.int64)).max(0)
    big = lambda a, b: diff_v(a, b, mv, spb) > np.float32(0.2) if a > b else diff_v(a, b, mv, spb) < np.float32(-0.2)
    # the smallest step the dead band lets through, if the scale leaves it inside (0, 0.2]
    small = next((c for c in range(1, 32768) if diff_v(c, 0, mv, spb) > 0), None)
    if small is not None and not (0 < diff_v(small, 0, mv, spb) <= np.float32(0.2) and 0 > diff_v(-small, 0, mv, spb) >= np.float32(-0.2)):
        small = None
    classes = [c for c in NEW_SHAPES if c != "D-small" or small is not None]

    def live(r, t):
        a, b = max(r - 3 * max(spb, 19), 0), min(r + 3 * max(spb, 19), nrows)
        return np.abs(rows0[a:b, t].astype(np.int64)).max() > 0.3 * peak[t]

    def place(cls, r, t, seam, anchor):
        """the shape's first row at r (anchor 0), or - D-long - its flat run across row r"""
        A = int(min(32767, max(0.8 * peak[t], 1)))
        sg = 1 if rng.random() < 0.5 else -1
        v = [-sg * A, -sg * A]                                   # two rows in front: the step that arms starts from a flat bottom
        if cls == "D-long":
            L = int(rng.integers(130, 401))
            v += [sg * A] * (L + 1) + [-sg * A]
            r0 = r - 2 - int(rng.integers(1, L)) if anchor else r - 2
        elif cls == "D-rearm":
            if not (big(0, -A) and big(A, 0)):
                return
            v += [0] * int(rng.integers(2, 8)) + [sg * A] * int(rng.integers(2, 8)) + [0, -sg * A]
            r0 = r - 2 - (int(rng.integers(1, len(v) - 3)) if anchor else 0)
        else:
            c = small + int(rng.integers(0, 2))
            if not (0 < diff_v(c, 0, mv, spb) <= np.float32(0.2)) or A - c < 1:
                c = small
            hi, lo = sg * A, sg * (A - c)
            v += [hi] * int(rng.integers(2, 7)) + [lo] * int(rng.integers(2, 6)) + [hi] * int(rng.integers(2, 5)) + [-sg * A]
            r0 = r - 2 - (int(rng.integers(1, len(v) - 3)) if anchor else 0)
        r1 = r0 + len(v)
        if r0 < 4 or r1 + 4 >= nrows or busy[max(r0 - spb, 0):r1 + spb, t].any():
            return
        old[:] = [s for s in old if s["trk"] != t or s["ext"][1] < r0 - 2 or s["ext"][0] > r1 + 2]
        rows[r0:r1, t] = v
        busy[max(r0 - 2, 0):r1 + 2, t] = True
        sites.append(dict(row=int(r0 + 2), trk=int(t), shape=cls, seam=seam, sign=sg, lo=int(r0), hi=int(r1 - 1)))

    spans = zs.burst_spans(bursts, nrows, zs.tail_rows(hdr))
    for seam, at in seam_rows(spans, ntrks).items():
        for r in at:
            for _ in range(per_seam):
                t = int(rng.integers(0, ntrks))
                tape_start = seam == "dz_head" and r == KDZ_HEAD      # (the tape's first burst starts exactly: no quiet zone to keep)
                if 4 <= r < nrows - 4 and (tape_start or live(r, t)):
                    place(str(rng.choice(classes)), int(r), t, seam, True)
                elif 4 <= r < nrows - 8 and not busy[r - 4:r + 8, t].any() and not any(s["trk"] == t and s["ext"][0] <= r + 8 and s["ext"][1] >= r - 4 for s in old):      # a quiet zone: exact zeros and a +-1 flicker leave the burst table alone
                    rows[r - 3:r + 3, t] = [0, 1, 0, 0, -1, 0]
                    busy[r - 4:r + 8, t] = True
                    sites.append(dict(row=int(r), trk=int(t), shape="Z-zero", seam=seam, sign=1, lo=int(r - 3), hi=int(r + 2)))
    for cls in classes:
        for _ in range(nrandom):
            t = int(rng.integers(0, ntrks))
            r = int(rng.integers(KDZ_HEAD, max(KDZ_HEAD + 1, nrows - 600)))
            if live(r, t) and live(r + 400 if cls == "D-long" else r, t):
                place(cls, r, t, "random", False)
    return rows.astype(np.int16), [{k: v for k, v in s.items() if k != "ext"} for s in old] + sites


def shaped(seed, scan, ntrks=None, **over):
    """(hdr, rows0, rows, sites, oracle options) of tape `seed`: zeros_shapes' tape and shapes for -zeros -differentiate, the new classes added.
    scan(hdr, rows, **cfgkw) -> the burst table.  Odd seeds: twice the speed in the header (samples_per_bit < 10: D-small exists)"""
    d = zs.draw(seed)
    d.update(over)
    hdr, rows0, opts = zs.base_tape(d["kind"], seed, d["noise_mv"], d["maxvolts"], ntrks=ntrks)
    if seed & 1:
        hdr = dataclasses.replace(hdr, ips=hdr.ips * 2)
    rows1, sites = zs.shape_rows(hdr, rows0, scan(hdr, rows0), np.random.default_rng(seed * 7919 + 17), diff=True, density=d["density"])
    rows, sites = add_shapes(hdr, rows0, rows1, sites, scan(hdr, rows1, differentiate=True), np.random.default_rng(seed * 104729 + 5))
    return hdr, rows0, rows, sites, opts + ["-zeros", "-differentiate"]


def skew_opt(ntrks, seed):
    """-skew= with a 50 on one track and zeros elsewhere"""
    d = [0] * ntrks
    d[seed % ntrks] = 50
    return "-skew=" + ",".join(str(x) for x in d)


# ---- path against path ----

def scan_pair(make_fe, hdr, rows, monkeypatch, **cfgkw):
    """(k_diffz's scan, k_decode's) of the same rows"""
    from readtape_amd import frontend
    out = []
    for knob in (None, "0"):
        monkeypatch.delenv(KNOB, raising=False)
        if knob is not None:
            monkeypatch.setenv(KNOB, knob)
        fe = make_fe(frontend.FrontEndConfig.from_header(hdr, find_zeros=True, differentiate=True, **cfgkw))
        assert fe.detector_path == ("diffzeros" if knob is None else "sample")
        out.append(fe.scan(rows).fetch())
    monkeypatch.delenv(KNOB, raising=False)
    return out


def square_rows(ntrks, nrows, first, last, period=16, amp=12000, seed=3):
    """a tape of its own for the block-length cases: square waves of `period` rows (every edge arms and confirms; the flat rows between are exact zeros) on rows
    [first, last], every track with a phase of its own, dead quiet elsewhere"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((nrows, ntrks), np.int16)
    n = np.arange(first, last + 1)
    for t in range(ntrks):
        ph = int(rng.integers(0, period))
        rows[first:last + 1, t] = np.where(((n + ph) // (period // 2)) % 2 == 0, amp, -amp)
    return rows


# ---- the cases both test files run (make_fe(cfg) -> a front end: the emulator's or the device's) ----

F_UNSAFE, F_EVENT_OVERFLOW, F_STATE_AT_END = 2, 4, 64


def base_hdr(ntrks, kind="pe"):
    hdr = zs.base_tape(kind, 1, 0.0, 2.5)[0]
    return dataclasses.replace(hdr, ntrks=ntrks)


def check_paths_reported(make_fe, monkeypatch):
    """detector_path is what rtfe_create decided: k_diffz for -zeros -differentiate, the sample path behind RTFE_DIFFZ_KERNEL=0, the others as they were"""
    from readtape_amd import frontend
    monkeypatch.delenv(KNOB, raising=False)
    cfg = frontend.FrontEndConfig.from_header
    nrzi, pe = base_hdr(9, "nrzi9"), base_hdr(9, "pe")
    for hdr in (nrzi, pe, base_hdr(9, "gcr"), base_hdr(7, "nrzi7")):
        assert make_fe(cfg(hdr, find_zeros=True, differentiate=True)).detector_path == "diffzeros"
        assert make_fe(cfg(hdr, find_zeros=True, differentiate=True, invert=True, skew=[50] + [0] * (hdr.ntrks - 1))).detector_path == "diffzeros"
    assert make_fe(cfg(pe, find_zeros=True)).detector_path == "zeros"
    assert make_fe(cfg(nrzi)).detector_path == "peak"
    assert make_fe(cfg(pe)).detector_path == "dense"
    assert make_fe(cfg(pe, differentiate=True)).detector_path == "sample"
    monkeypatch.setenv(KNOB, "0")
    assert make_fe(cfg(pe, find_zeros=True, differentiate=True)).detector_path == "sample"
    assert make_fe(cfg(pe, find_zeros=True)).detector_path == "zeros"
    monkeypatch.delenv(KNOB, raising=False)


MODES = ("plain", "invert", "skew")
SEEDS = range(2000, 2014)


def check_against_oracle(mode, make_fe, fe_factory, tmp_path, seeds=SEEDS):
    """the shaped tapes end to end against the oracle (transitions and .tap bytes); the coverage the seeds must reach, asserted"""
    from readtape_amd import frontend

    def bursts(hdr, rows, **kw):
        return make_fe(frontend.FrontEndConfig.from_header(hdr, find_zeros=True, **kw)).scan(rows).fetch(events=False).bursts
    cov, changed = {}, 0
    for seed in seeds:
        hdr, rows0, rows, sites, opts = shaped(seed, bursts)
        extra = {"plain": [], "invert": ["-invert"], "skew": [skew_opt(hdr.ntrks, seed)]}[mode]
        msgs, b = zs.e2e(hdr, rows, opts + extra, str(tmp_path / f"s{seed}"), fe_factory)
        assert not msgs, f"seed {seed} {zs.draw(seed)} {opts + extra}: " + "\n".join(str(m) for m in msgs[:8])
        _, b0 = zs.e2e(hdr, rows0, opts + extra, str(tmp_path / f"u{seed}"), fe_factory)
        changed += b.size != b0.size or not np.array_equal(b["timenow_ns"], b0["timenow_ns"])
        for k, v in coverage(sites, hdr, rows.shape[0], bursts(hdr, rows, differentiate=True)).items():
            cov[k] = cov.get(k, 0) + v
    for c in zs.DIFF_SHAPES + NEW_SHAPES + SEAMS:
        assert cov.get(c, 0) >= 3 * MIN_SEAMS, (c, cov)
    assert changed >= len(seeds) // 2, "the shapes did not change what the oracle decodes"
    return cov


def same_pair(make_fe, hdr, rows, monkeypatch, **cfgkw):
    import zeros_util
    a, b = scan_pair(make_fe, hdr, rows, monkeypatch, **cfgkw)
    zeros_util.same_scan(b, a, hdr.ntrks)
    return a


def check_track_counts(ntrks, make_fe, monkeypatch):
    from readtape_amd import frontend

    def bursts(hdr, rows, **kw):
        return make_fe(frontend.FrontEndConfig.from_header(hdr, find_zeros=True, **kw)).scan(rows).fetch(events=False).bursts
    for seed, kw in ((4, {}), (5, {"invert": True}), (6, {"skew": [(7 * t) % 51 for t in range(ntrks)]})):
        hdr, rows0, rows, sites, opts = shaped(seed, bursts, ntrks=ntrks, kind="pe")
        r = same_pair(make_fe, hdr, rows, monkeypatch, **kw)
        assert int(r.counts.sum()) > 100 * ntrks
        cov = coverage(sites, hdr, rows.shape[0], r.bursts)
        for c in ("dz_sub", "D-long", "D-rearm") + (("dz_chunk",) if rows.shape[0] > KDZ_HEAD + (chunk_subs(ntrks) + 1) * KDZ_SUB else ()):
            assert cov.get(c, 0) >= 1, (c, cov)


# where a block - and where the burst - ends against the head, a sub-segment and (19 tracks: 13 sub-segments a chunk) a chunk
def seam_positions(ntrks):
    ks = (1, 2, chunk_subs(ntrks), chunk_subs(ntrks) + 1)
    return [KDZ_HEAD + d for d in (-1, 0, 1)] + [KDZ_HEAD + k * KDZ_SUB + d for k in ks for d in (-1, 0, 1)]


def check_block_ends(ntrks, make_fe, monkeypatch):
    hdr = base_hdr(ntrks)
    for end in seam_positions(ntrks):
        # the block's last row at `end` - 1, dead quiet behind it (the burst runs on to the tape's end) ...
        r = same_pair(make_fe, hdr, square_rows(ntrks, end + 700, 8, end - 1, seed=end), monkeypatch)
        assert r.nbursts == 1 and int(r.bursts[0]["end_sample"]) == end + 700 and (r.counts[0, 0] > 0).all()
        # ... and the tape's: the burst stops there, mid-signal
        r = same_pair(make_fe, hdr, square_rows(ntrks, end, 8, end - 1, seed=end), monkeypatch)
        assert r.nbursts == 1 and int(r.bursts[0]["end_sample"]) == end


def check_flags(make_fe, monkeypatch):
    ntrks = 9
    hdr = base_hdr(ntrks)
    # a gap shorter than kMarginRows + 64: the zone search asks for more quiet rows than that before it cuts a tape, so the blocks stay one burst on both paths
    rows = square_rows(ntrks, 3000, 8, 2900)
    rows[1200:1500] = 0
    r = same_pair(make_fe, hdr, rows, monkeypatch)
    assert not int(r.bursts[-1]["flags"]) & F_EVENT_OVERFLOW
    # ... and a gap that makes a zone: a second burst, restarted kMarginRows in front of the zone's end
    rows = square_rows(ntrks, 4000, 8, 3900)
    rows[1200:2000] = 0
    r = same_pair(make_fe, hdr, rows, monkeypatch)
    assert r.nbursts == 2 and int(r.bursts[1]["reset_sample"]) == int(r.bursts[1]["zone_end"]) - zs.K_MARGIN_ROWS and not int(r.bursts[1]["flags"]) & F_UNSAFE
    # the tape ends with a crossing pending: the last edge arms, flat rows to the end
    rows = square_rows(ntrks, 1000, 8, 999, period=16)
    rows[990:] = rows[989]
    rows[995:, 3] = -rows[989, 3]
    r = same_pair(make_fe, hdr, rows, monkeypatch)
    assert int(r.bursts[0]["flags"]) & F_STATE_AT_END
    # the lists fill: flags and clamped counts equal, the events up to the cap
    r = same_pair(make_fe, hdr, square_rows(ntrks, 3000, 8, 2900), monkeypatch, events_per_sample_cap=0.01)
    assert int(r.bursts[0]["flags"]) & F_EVENT_OVERFLOW and (r.counts[0, 0] == int(r.bursts[0]["event_cap"])).all()


def check_long_flat(make_fe, monkeypatch):
    """70 000 flat rows between arming and confirmation: d1 >= 65536 does not fit the record - the slot is left unwritten and the burst flagged, on both
    paths.  Track 1's first event is that slot: nothing of its list is compared; track 0's list is whole"""
    import zeros_util
    hdr = base_hdr(2)
    n = 70000 + 600
    rows = square_rows(2, n, 8, n - 1)
    rows[:100, 1] = 0
    rows[100:70100, 1] = 12000
    a, b = scan_pair(make_fe, hdr, rows, monkeypatch)
    assert a.nbursts == b.nbursts == 1 and (a.counts == b.counts).all() and int(a.counts[0, 0, 1]) > 10
    for k in ("reset_sample", "safe_last", "end_sample", "flags"):
        assert (a.bursts[k] == b.bursts[k]).all(), k
    assert int(a.bursts[0]["flags"]) & F_EVENT_OVERFLOW
    assert a.track_events(0, 0, 0).tobytes() == b.track_events(0, 0, 0).tobytes()
    assert a.track_events(0, 0, 1)[1:].tobytes() == b.track_events(0, 0, 1)[1:].tobytes()      # (behind the slot: written by both)


def check_exact_scans(make_fe, monkeypatch):
    """rtfe_scan_exact - k_decode, the second implementation - of every burst's [reset_sample, end_sample) gives the scan's events"""
    from readtape_amd import frontend

    def bursts(hdr, rows, **kw):
        return make_fe(frontend.FrontEndConfig.from_header(hdr, find_zeros=True, **kw)).scan(rows).fetch(events=False).bursts
    monkeypatch.delenv(KNOB, raising=False)
    hdr, rows0, rows, sites, opts = shaped(2002, bursts, kind="gcr", noise_mv=0.0)
    fe = make_fe(frontend.FrontEndConfig.from_header(hdr, find_zeros=True, differentiate=True))
    assert fe.detector_path == "diffzeros"
    r = fe.scan(rows).fetch()
    assert r.nbursts >= 2
    for b in range(r.nbursts):
        x = fe.scan_exact(rows, int(r.bursts[b]["reset_sample"]), int(r.bursts[b]["end_sample"])).fetch()
        assert (x.counts[0] == r.counts[b]).all(), b
        for t in range(hdr.ntrks):
            assert x.track_events(0, 0, t).tobytes() == r.track_events(b, 0, t).tobytes(), (b, t)
