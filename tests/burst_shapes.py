"""Tapes that aim at the seams of the quiet map's producers and of the burst search, and the check that holds a scan's table against tests/burst_ref.py.

A tape is all-zero rows with single samples poked in; a shape says which groups of 64 rows stay quiet ("runs": first group, length - every other complete
group gets one sample of quiet_i + 1) and which further samples it pokes.  The decode behind the table is trivial.  G = gap_chunks; a word = 64 groups of
the quiet map; the burst search takes a thread per word and rounds of RTFE_BURSTS_WPR words (4096 by default).
The same cases run on the CPU emulator (tests/test_emul_burst_table.py) and on the device (tests/test_gpu_burst_table.py) through a make_fe argument."""
import itertools
from dataclasses import dataclass, field

import numpy as np

import burst_ref as ref
from readtape_amd import frontend

WPRS = (None, "1", "3", "64")           # the rounds knob: the single workgroup, and a workgroup per round of 1, 3 and 64 words
SIFT_GROUPS, DENSE_GROUPS = 14, 8       # groups of 64 rows per tile of k_sift / k_dseg

# what a poked sample's code stands for, given quiet_i
VALUES = {"+q": lambda q: q, "-q": lambda q: -q, "+q1": lambda q: q + 1, "-q1": lambda q: -(q + 1), "rail": lambda q: -32768, "+rail": lambda q: 32767}


def config(producer, ntrks=2, G=7, cap_frac=0.0, nparm=1):
    """A configuration that reaches one producer of the quiet map; quiet_volts and gap_min_samples are explicit so that burst_ref.derive stays short.
      peak   NRZI peak detection: k_sift / k_sift_s + k_qpack        dense_pe / dense_gcr   PE / GCR peak detection: k_dseg
      zeros  -zeros: k_quiet                                          diff   -differentiate: k_quiet, and the 0.024 V band is tighter than quiet_volts
      diffzeros  -zeros -differentiate: k_quiet, the band 0.24 V / samples per bit (tighter than quiet_volts)
      peak_invert  -invert: k_sift_s's general build at 7 and 9 tracks      peak_generic  RTFE_SIFT_GENERIC (ENV_OF): k_sift where k_sift_s would run"""
    kw = dict(ntrks=ntrks, maxvolts=5.0, ips=50.0, gap_min_samples=(G - 1) * 64, quiet_volts=0.01, events_per_sample_cap=cap_frac)
    nrzi = dict(mode=frontend.NRZI, bpi=800.0, tdelta_ns=2500, parmsets=list(frontend.DEFAULT_PARMSETS[frontend.NRZI][:nparm]))
    if producer in ("peak", "peak_generic"):
        return frontend.FrontEndConfig(**nrzi, **kw)
    if producer == "peak_invert":
        return frontend.FrontEndConfig(invert=True, **nrzi, **kw)
    if producer == "diffzeros":
        kw["quiet_volts"] = 0.05
        return frontend.FrontEndConfig(find_zeros=True, differentiate=True, **nrzi, **kw)
    if producer == "zeros":
        return frontend.FrontEndConfig(find_zeros=True, **nrzi, **kw)
    if producer == "diff":
        kw["quiet_volts"] = 0.05
        return frontend.FrontEndConfig(differentiate=True, **nrzi, **kw)
    if producer == "dense_pe":
        return frontend.FrontEndConfig(mode=frontend.PE, bpi=1600.0, tdelta_ns=1250, parmsets=list(frontend.DEFAULT_PARMSETS[frontend.PE][:nparm]), **kw)
    if producer == "dense_gcr":
        return frontend.FrontEndConfig(mode=frontend.GCR, bpi=9042.0, tdelta_ns=221, parmsets=list(frontend.DEFAULT_PARMSETS[frontend.GCR][:nparm]), **kw)
    raise ValueError(producer)


PATH_OF = {"peak": "peak", "peak_invert": "peak", "peak_generic": "peak", "zeros": "zeros", "diff": "sample", "diffzeros": "diffzeros", "dense_pe": "dense", "dense_gcr": "dense"}
ENV_OF = {"peak_generic": {"RTFE_SIFT_GENERIC": "1"}}


@dataclass
class Shape:
    name: str
    ngroups: int                         # complete groups
    runs: list                           # (first group, length) of the quiet runs; every other complete group is loud
    tail_rows: int = 0                   # rows of the incomplete last group
    pokes: list = field(default_factory=list)      # further samples (row, track, code of VALUES)
    G: int = 7
    producer: str = "zeros"
    ntrks: int = 2
    nparm: int = 1
    cap_frac: float = 0.0
    first: bool = True                   # first_is_tape_start
    own_groups: int = 0                  # own_rows = 64 * own_groups + own_off (0: no halo)
    own_off: int = 0
    overflow_last: int = 0               # an event capacity that the last so many regions do not fit
    expect: dict = field(default_factory=dict)      # what the shape is meant to show, asserted on the REFERENCE's table (the shape does what it says)

    @property
    def nrows(self):
        return 64 * self.ngroups + self.tail_rows

    def cfg(self):
        return config(self.producer, self.ntrks, self.G, self.cap_frac, self.nparm)

    def all_pokes(self):
        quiet = set()
        for g0, n in self.runs:
            quiet.update(range(g0, g0 + n))
        loud = [(64 * g + (7 * g) % 64, g % self.ntrks, "+q1") for g in range(self.ngroups) if g not in quiet]
        return loud + list(self.pokes)

    def rows(self, quiet_i):
        rows = np.zeros((self.nrows, self.ntrks), dtype=np.int16)
        for r, t, code in self.all_pokes():
            rows[r, t] = VALUES[code](quiet_i)
        return rows


# ------------------------------------------------------------------------------------------------ the shapes
def zone_length_shapes():
    """Runs of exactly G - 1, G and G + 1 quiet groups whose last group is bit 0, 1, 62 or 63 of a word (so the first lies in the same word, the previous one
    or - G = 130 - two words back), for the default floor G = 7, both sides of the bit-trick / walk split (63, 64, 65) and a walk across two words (130).
    The end words step through every residue of a round of three words."""
    out = []
    for G in (7, 63, 64, 65, 130):
        stride = G // 64 + 4
        runs, want = [], 0
        for k, (L, bit) in enumerate(itertools.product((G - 1, G, G + 1), (0, 1, 62, 63))):
            last = 64 * ((k + 1) * stride + (k - (k + 1) * stride) % 3) + bit          # (word % 3 == k % 3)
            runs.append((last - L + 1, L))
            want += L >= G
        ngroups = runs[-1][0] + runs[-1][1] + 1
        assert all(a[0] + a[1] < b[0] for a, b in zip(runs, runs[1:])) and runs[0][0] > 0
        assert {((r[0] + r[1] - 1) // 64) % 3 for r in runs} == {0, 1, 2}
        out.append(Shape(f"zone_length_G{G}", ngroups, runs, G=G, expect=dict(zones=want, exact=True)))
    return out


def tape_start_shapes():
    """The tape begins with G - 1 quiet groups (an exact-start burst), with G (none: it begins inside a zone), or loud - each with first_is_tape_start on and off."""
    out = []
    for first in (True, False):
        for name, head, exact in (("short_of_a_zone", 6, True), ("a_zone", 7, False), ("loud", 0, True)):
            runs = ([(0, head)] if head else []) + [(20, 8)]
            out.append(Shape(f"tape_start_{name}_first{int(first)}", 40, runs, first=first, expect=dict(zones=1 + (head >= 7), exact=exact and first)))
    return out


def tape_end_shapes():
    """nrows % 64 and (nrows // 64) % 64 in {0, 1, 63}; quiet up to the end (a zone ends with the map's last group), the last complete group loud, the incomplete
    tail loud behind a quiet group."""
    out = []
    for rem, gw in itertools.product((0, 1, 63), (0, 1, 63)):
        n = 128 if gw == 0 else 64 + gw
        out.append(Shape(f"tape_end_quiet_rem{rem}_g{gw}", n, [(3, 9), (n - 8, 8)], tail_rows=rem, expect=dict(zones=2, last_zone_end=64 * n)))
        out.append(Shape(f"tape_end_short_rem{rem}_g{gw}", n, [(3, 9), (n - 6, 6)], tail_rows=rem, expect=dict(zones=1)))
        out.append(Shape(f"tape_end_loud_group_rem{rem}_g{gw}", n, [(3, 9), (n - 9, 8)], tail_rows=rem, expect=dict(zones=2, last_zone_end=64 * (n - 1))))
        if rem:
            out.append(Shape(f"tape_end_loud_tail_rem{rem}_g{gw}", n, [(3, 9), (n - 8, 8)], tail_rows=rem, pokes=[(64 * n + rem - 1, 1, "rail")],
                             expect=dict(zones=2, last_zone_end=64 * n)))
    return out


def producer_end_shapes():
    """The end of the tape through the producers that make the map a tile at a time (k_sift, k_sift_s, k_dseg): the last tile is whole, holds one group or lacks
    one (126, 127, 128 groups against tiles of 14 and of 8), with and without an incomplete last group behind it; quiet up to the end, and G - 1 quiet groups
    short of a zone - an incomplete group taken for quiet would make it one."""
    out = []
    for (producer, ntrks), n, rem in itertools.product((("peak", 2), ("peak", 9), ("dense_pe", 2), ("dense_pe", 9), ("dense_gcr", 9)), (126, 127, 128), (0, 1, 63)):
        kw = dict(tail_rows=rem, producer=producer, ntrks=ntrks)
        out.append(Shape(f"end_quiet_{producer}_{ntrks}trk_{n}groups_rem{rem}", n, [(3, 9), (n - 8, 8)], expect=dict(zones=2, last_zone_end=64 * n), **kw))
        out.append(Shape(f"end_short_{producer}_{ntrks}trk_{n}groups_rem{rem}", n, [(3, 9), (n - 6, 6)], expect=dict(zones=1), **kw))
    return out


def long_zone_shapes():
    """A zone of more than 64 words that ends at bit 63 of word 65 (the last word of a round of three) and at bit 0 of word 66 (the first).  Where the round that holds
    its end begins at word 65 or 66 - rounds of one word, and of three for the second shape - the zone's start in word 0 lies in front of the look-back window and
    is found in HBM."""
    return [Shape("long_zone_end_bit63", 64 * 66 + 6, [(10, 64 * 66 - 10)], expect=dict(zones=1, last_zone_end=64 * 64 * 66)),
            Shape("long_zone_end_bit0", 64 * 66 + 7, [(10, 64 * 66 + 1 - 10)], expect=dict(zones=1, last_zone_end=64 * (64 * 66 + 1)))]


MANY = 1040


def many_bursts_shape():
    """More than 1024 bursts, each G quiet groups and one loud group: the second round of the 1024-wide loops of br_tail and k_pack_plan; 130 words of the map, a zone
    end in every word (the first and the last word of every round, whatever the rounds knob).  Every 40th loud group holds a full-scale square wave of 2 .. 6 periods
    (NRZI peak detection: two events a period), so that the lists are not all empty."""
    runs = [(1 + 8 * k, 7) for k in range(MANY)]
    pokes = []
    for k in range(0, MANY, 40):
        r = 64 * (8 + 8 * k) + 8
        for i in range(8 * (2 + k // 40 % 5)):                    # a square wave of 2 .. 6 periods of eight rows
            pokes.append((r + i, 0, "+rail" if i % 8 < 4 else "rail"))
    return Shape("many_bursts", 1 + 8 * MANY, runs, pokes=pokes, producer="peak", expect=dict(zones=MANY, exact=True))


def event_region_shapes():
    """events_per_sample_cap = 0.7 and bursts of 960 rows: float32(960) * float32(0.7) is 672 exactly, the double product of the same two numbers 671.99998...;
    two parameter sets; an event capacity that the last three regions do not fit."""
    runs = [(1 + 11 * k, 10) for k in range(12)]
    return [Shape("event_regions_f32", 1 + 11 * 12 + 3, runs, cap_frac=0.7, nparm=2, expect=dict(zones=12, f32_differs=True)),
            Shape("event_regions_overflow", 1 + 11 * 12 + 3, runs, cap_frac=0.7, nparm=2, overflow_last=3, expect=dict(zones=12, overflow=3))]


def shard_seam_shapes():
    """own_rows < nrows.  A zone that straddles the seam and ends one group short of own_rows + 64 G (ours: the neighbour sees too few quiet groups), at it and one
    group behind it (the neighbour's); a halo without any zone (TRUNCATED); an exact-start burst with a halo, alone and with others."""
    out, own, G = [], 30, 7
    for d, owned in ((-1, 3), (0, 2), (1, 2)):
        end = own + G + d
        out.append(Shape(f"shard_seam_zone_end_{d:+d}", 60, [(2, 10), (25, end - 25), (45, 10)], own_groups=own, expect=dict(owned=owned, total=owned + 1, truncated=False)))
        out.append(Shape(f"shard_seam_zone_end_{d:+d}_first0", 60, [(2, 10), (25, end - 25), (45, 10)], own_groups=own, first=False,
                         expect=dict(owned=owned - 1, total=owned, truncated=False)))
    for d, owned in ((-1, 3), (0, 2)):          # own_rows = 64 * 30 - 63: the bound own_rows + 64 G lies one row behind group 36's end
        out.append(Shape(f"shard_seam_unaligned_zone_end_{d:+d}", 60, [(2, 10), (25, own + G + d - 25), (45, 10)], own_groups=own, own_off=-63,
                         expect=dict(owned=owned, total=owned + 1, truncated=False)))
    out.append(Shape("shard_seam_last_zone_straddles", 60, [(2, 10), (25, own + G - 1 - 25)], own_groups=own, expect=dict(owned=3, total=3, truncated=True)))
    out.append(Shape("shard_seam_empty_halo", 60, [(2, 10), (15, 8)], own_groups=own, expect=dict(owned=3, total=3, truncated=True)))
    out.append(Shape("shard_seam_only_exact_start", 60, [], own_groups=own, expect=dict(owned=1, total=1, truncated=True)))
    out.append(Shape("shard_seam_zone_at_row0", 60, [(0, 9), (45, 10)], own_groups=own, expect=dict(owned=1, total=2, truncated=False)))
    return out


def threshold_shape(producer, ntrks):
    """Zones of exactly G groups with ONE sample poked into a group of each: +quiet_i and -quiet_i leave the zone standing, quiet_i + 1, -(quiet_i + 1) and -32768
    remove it.  The sample sits on the first or the last track of row 0 or row 63, or is the last sample inside / the first behind the group's first 128 bytes
    (k_quiet looks at those first); its group is the last of a k_sift tile or the first of the next one (groups 13 and 14: the k_qpack seam), for k_dseg
    groups 7 and 8 of its tiles of eight."""
    G, runs, pokes, cur, stand = 7, [], [], 1, 0
    tile = DENSE_GROUPS if producer.startswith("dense") else SIFT_GROUPS          # (k_dseg: the last group of a tile of eight and the first of the next)
    places = [(0, 0), (0, ntrks - 1), (63, 0), (63, ntrks - 1), (63 // ntrks, 63 % ntrks), (64 // ntrks, 64 % ntrks)]
    for (row, trk), code, tile_group in itertools.product(places, ("+q", "-q", "+q1", "-q1", "rail"), (tile - 1, 0)):
        g = cur + 3
        while g % tile != tile_group:
            g += 1
        runs.append((g - 3, G))
        pokes.append((64 * g + row, trk, code))
        stand += code in ("+q", "-q")
        cur = g - 3 + G + 1
    return Shape(f"threshold_{producer}_{ntrks}trk", cur + 1, runs, pokes=pokes, producer=producer, ntrks=ntrks, expect=dict(zones=stand, exact=True))


TABLE_SHAPES = zone_length_shapes() + tape_start_shapes() + tape_end_shapes() + long_zone_shapes() + event_region_shapes() + shard_seam_shapes()
PRODUCER_END_SHAPES = producer_end_shapes()
THRESHOLD_CASES = [(p, n) for p in ("peak", "dense_pe", "dense_gcr", "zeros", "diff", "diffzeros") for n in (2, 9, 19)] + [("peak_invert", 9), ("peak_generic", 9)]


# ------------------------------------------------------------------------------------------------ the check
def set_wpr(monkeypatch, wpr):
    if wpr is None:
        monkeypatch.delenv("RTFE_BURSTS_WPR", raising=False)
    else:
        monkeypatch.setenv("RTFE_BURSTS_WPR", wpr)


def check_expectations(shape, ent, n_owned, n_total, gap_chunks):
    """The shape does what its name says - asserted on the reference's table alone."""
    e = shape.expect
    exact = [x for x in ent if x["flags"] & ref.F_EXACT_START]
    if "zones" in e and not shape.own_groups:
        assert len(ent) - len(exact) == e["zones"], (len(ent), len(exact))
    if "exact" in e:
        assert bool(exact) == e["exact"]
    if "last_zone_end" in e:
        assert ent[-1]["zone_end"] == e["last_zone_end"]
    if "owned" in e:
        assert (n_owned, n_total) == (e["owned"], e["total"]), (n_owned, n_total)
        assert bool(n_owned and ent[n_owned - 1]["flags"] & ref.F_TRUNCATED) == e["truncated"]
    if e.get("f32_differs"):
        assert any(x["cap_f64"] != x["event_cap"] for x in ent)
    if "overflow" in e:
        flagged = [bool(x["flags"] & ref.F_EVENT_OVERFLOW) for x in ent]
        assert flagged == [False] * (len(ent) - e["overflow"]) + [True] * e["overflow"]
        assert all(x["event_cap"] == 0 for x in ent[-e["overflow"]:]) and all(a["event_base"] < b["event_base"] for a, b in zip(ent, ent[1:]))


def scan_table(fe, rows, nrows, first, own_rows, event_capacity=None):
    """One scan; returns (result, nbursts_total, the event capacity it ran with)."""
    b = fe._buffers(nrows)
    if event_capacity is not None:
        assert event_capacity <= b["cap"]
        b = dict(b, cap=int(event_capacity))          # (the arena stays as large as it was: only what the scan is told shrinks)
        fe._cache[("scan", nrows)] = b
    r = fe.scan(rows, first_is_tape_start=first, own_rows=own_rows).fetch(events=False)
    total = int(fe.backend.to_numpy(b["ws"][:16], np.dtype(np.int32))[2])          # BurstScratch::nbursts_total
    return r, total, b["cap"]


def check_handle(fe, cfg, expect_path=None):
    """quiet_i, gap_chunks and cap_frac for a handle, gap_chunks cross-checked against rtfe_max_bursts at two row counts."""
    quiet_i, G, cap_frac = ref.derive(cfg)
    for n in (64 * 1000 + 17, 64 * 123457):
        assert int(fe.lib.rtfe_max_bursts(fe.h, n)) == (n // 64) // G + 4, (n, G)
    if expect_path is not None:
        assert fe.detector_path == expect_path, fe.detector_path
    return quiet_i, G, cap_frac


def check_shape(shape, make_fe, monkeypatch, wpr):
    """A fresh handle for the setting of the rounds knob (a handle reads it when it is made), one scan, every burst against the reference."""
    set_wpr(monkeypatch, wpr)
    cfg = shape.cfg()
    for k, v in ENV_OF.get(shape.producer, {}).items():
        monkeypatch.setenv(k, v)
    fe = make_fe(cfg)
    try:
        quiet_i, G, cap_frac = check_handle(fe, cfg, PATH_OF[shape.producer])
        assert G == shape.G
        rows = shape.rows(quiet_i)
        nrows, own = shape.nrows, (64 * shape.own_groups + shape.own_off if shape.own_groups else shape.nrows)
        maxb = int(fe.lib.rtfe_max_bursts(fe.h, nrows))
        loud = ref.loud_groups_of_rows(rows, quiet_i)
        assert loud == ref.loud_groups_of_pokes([(r, t, VALUES[c](quiet_i)) for r, t, c in shape.all_pokes()], nrows, quiet_i)
        lists = len(cfg.parmsets) * cfg.ntrks
        capacity = None
        if shape.overflow_last:
            ent, _, _ = ref.table(loud, nrows, G, cap_frac, len(cfg.parmsets), cfg.ntrks, shape.first, own, 1 << 62, maxb)
            x = ent[-shape.overflow_last]
            capacity = x["event_base"] + x["event_cap"] * lists - 1
        r, total, cap = scan_table(fe, rows, nrows, shape.first, own, capacity)
        ent, n_owned, n_total = ref.table(loud, nrows, G, cap_frac, len(cfg.parmsets), cfg.ntrks, shape.first, own, cap, maxb)
        check_expectations(shape, ent, n_owned, n_total, G)
        ref.compare(ent, n_owned, n_total, r.bursts, r.next_burst if n_total > n_owned else None, total)
        return fe, r, ent
    except BaseException:
        fe.close()
        raise


def check_table(shape, make_fe, monkeypatch, wpr):
    fe, r, ent = check_shape(shape, make_fe, monkeypatch, wpr)
    fe.close()


def check_many_bursts(make_fe, monkeypatch, wpr):
    """... and with more than 1024 bursts the packed fetch: rtfe_pack_events' plan against the reference's, every packed list against the unpacked fetch."""
    shape = many_bursts_shape()
    monkeypatch.setenv("RTFE_PACK_EVENTS", "0")
    fe, r, ent = check_shape(shape, make_fe, monkeypatch, wpr)
    try:
        nb, T = r.nbursts, shape.ntrks
        assert nb == MANY + 1
        r.fetch()                                              # the arena as it is
        plain = [[r.track_events(b, 0, t).copy() for t in range(T)] for b in range(nb)]
        assert r.counts.max() > 1, "the shape is meant to leave lists of several events"
        cap2, bases, total = ref.pack_plan(r.counts.reshape(nb, -1), [e["event_cap"] for e in ent[:nb]])
        monkeypatch.setenv("RTFE_PACK_EVENTS", "1")
        r.fetch()                                              # packs on the device, re-bases the host copy of the table
        assert r.packed
        plan = fe.backend.to_numpy(r.bufs["plan"], frontend.PLAN_DTYPE)[: nb + 1]
        assert [int(x) for x in plan["event_cap"][:nb]] == cap2
        assert [int(x) for x in plan["event_base"][:nb]] == bases
        assert (int(plan["event_base"][nb]), int(plan["reserved"][nb])) == (total, nb)
        assert [int(x) for x in r.bursts["event_base"]] == bases and [int(x) for x in r.bursts["event_cap"]] == cap2
        for b in range(nb):
            for t in range(T):
                assert r.track_events(b, 0, t).tobytes() == plain[b][t].tobytes(), (b, t)
    finally:
        fe.close()


def check_threshold(producer, ntrks, make_fe, monkeypatch):
    fe, r, ent = check_shape(threshold_shape(producer, ntrks), make_fe, monkeypatch, None)
    fe.close()


# ------------------------------------------------------------------------------------------------ the shape only the device can afford
BIG_GROUPS = (1 << 24) // 64 + 128      # 2^24 + 8192 rows of two tracks, 67 MB: 4098 words of the map - the single workgroup's own loop runs a second round
BIG_VARIANTS = {                         # where the long zone that begins in word 4000 ends
    "straddles_4095_4096": 64 * 4096 + 9,        # ... inside word 4096: it straddles the rounds' seam
    "ends_bit0_of_4096": 64 * 4096,
    "ends_bit63_of_4095": 64 * 4096 - 1}


def big_shape(variant):
    """A zone of 96 words that begins in word 4000 - in front of the second round's look-back window, so its start is found in HBM - and ends around the seam of
    words 4095 / 4096; a zone that lies in front of it, one that begins at bit 20 of word 4096, one that ends with the map."""
    last = BIG_VARIANTS[variant]
    first = 64 * 4000 + 50
    runs = [(64 * 100 + 5, 20), (first, last - first + 1), (64 * 4096 + 20, 10), (BIG_GROUPS - 8, 8)]
    return Shape(f"big_{variant}", BIG_GROUPS, runs, expect=dict(zones=4, exact=True, last_zone_end=64 * BIG_GROUPS))


def check_big(make_fe, monkeypatch):
    """The rows are made and poked on the device; the reference works on the poked positions and never sees a host copy of the rows.  Prints the device time of
    k_quiet and k_bursts per scan (reported, not asserted)."""
    import torch
    set_wpr(monkeypatch, None)
    cfg = big_shape("straddles_4095_4096").cfg()
    fe = make_fe(cfg)
    try:
        quiet_i, G, cap_frac = check_handle(fe, cfg, "zeros")
        nrows = 64 * BIG_GROUPS
        maxb = int(fe.lib.rtfe_max_bursts(fe.h, nrows))
        rows = torch.zeros((nrows, cfg.ntrks), dtype=torch.int16, device="cuda")
        have = {}
        fe.set_timing(True)
        for variant in BIG_VARIANTS:
            shape = big_shape(variant)
            want = {(r, t): VALUES[c](quiet_i) for r, t, c in shape.all_pokes()}
            delta = [(r, t, v) for (r, t), v in want.items() if have.get((r, t)) != v] + [(r, t, 0) for (r, t) in have if (r, t) not in want]
            d = np.array(delta, dtype=np.int64)
            rows[torch.from_numpy(d[:, 0]).cuda(), torch.from_numpy(d[:, 1]).cuda()] = torch.from_numpy(d[:, 2].astype(np.int16)).cuda()
            have = want
            loud = ref.loud_groups_of_pokes([(r, t, v) for (r, t), v in want.items()], nrows, quiet_i)
            r, total, cap = scan_table(fe, rows, nrows, True, nrows)
            ms, scans = fe.kernel_ms()
            print(f"{shape.name}: {nrows} rows, k_quiet {ms['k_quiet']:.3f} ms, k_bursts {ms['k_bursts']:.3f} ms, {r.nbursts} bursts")
            ent, n_owned, n_total = ref.table(loud, nrows, G, cap_frac, len(cfg.parmsets), cfg.ntrks, True, nrows, cap, maxb)
            check_expectations(shape, ent, n_owned, n_total, G)
            ref.compare(ent, n_owned, n_total, r.bursts, None, total)
    finally:
        fe.close()
