"""The amplitude shapes of tests/fuzz_util.py written ON the seams of the peak path (k_sift_s / k_sift -> k_prep -> k_clear -> k_gain -> k_gain_seg ->
k_gain_join -> k_emit_seg) and of the dense path (k_dseg -> k_dchain): the inputs of tools/fuzz_shapes.py --seams and of tests/test_*_seam_shapes.py.
Test infrastructure.

Neither path decides from samples: they decide from records, margins, bit-planes and guessed states, and they cut the tape into tiles, strips, runs,
segments, sub-segments and rounds.  fuzz_util.shape_rows writes its mixture over random peaks of short blocks (no track of its NRZI tapes has a second
segment, and no test says that a shape met a tile edge); rail_shapes writes one shape, the code -32768, on the seams.  Here six named shapes - a plateau,
a double top or bottom, a valley behind a flat top, a stale minimum, a notch in a shoulder, a weak run - are written so that samples of the shape lie on
BOTH sides of a cut: the plateau runs across it, the two tops of a double lie either side of it, the stale minimum's owner lies in the tile in front of
its candidate.  The cuts counted in rows are mirrored from the sources (rail_shapes' constants, and kernel_constants() here for the rest: a retune fails
tests/test_emul_seam_shapes.py); the cuts counted in records (k_gain_seg's segments, k_emit_seg's rounds) cannot be known from the samples: the generator
shapes every peak of a stretch around each multiple of the segment length, and the tests take what the segments met from the emulator's seg_shapes: line.
The NRZI tapes have one block of some 2 000 bytes: at least four default segments per track.  No sample of a shape is -32768.  Deterministic per seed."""
import os
import re

import numpy as np

import fuzz_util
import rail_shapes as rs
from rail_shapes import K_DS_SUB, K_DS_TILE, K_PK_BACK, K_SF_STRIP, K_SF_TILE, PK_SEG_RECS, PREP_RUN, seams_of, sift_halos, window  # noqa: F401
from readtape_amd import synth, tbin

SHAPES = ("A-plateau", "A-double", "A-valley", "A-stale", "A-notch", "A-weak")
ROW_SEAMS = ("sift_tile", "sift_halo", "sift_strip", "sift_part", "sift_pstrip", "prep_run", "dseg_sub", "dseg_tile", "dseg_warm")
PEAK_SEAMS = ("sift_tile", "sift_halo", "sift_strip", "sift_part", "sift_pstrip", "prep_run")       # the cuts of the peak path (NRZI)
DENSE_SEAMS = ("dseg_sub", "dseg_tile", "dseg_warm")                                                # ... of the dense path (GCR, PE)
KINDS = ("nrzi9", "nrzi7", "nrzi9_m", "gcr", "gcr_m", "pe")
ES_ROUND = 64                                                          # records a wave of k_emit_seg takes at a time
SEG_COUNTS = ("planned", "standing", "refused", "stopped", "rejoined", "nc_first", "nc_last", "nc_warm", "nc_near", "back_any", "back_cross", "round_edge", "weak", "unknown")


def kernel_constants(root):
    """rail_shapes.kernel_constants and what this generator mirrors beside it: the last head's split in k_sift_s, k_dseg's warm-up rows, k_emit_seg's rounds,
    the look-back's bound in k_gain's general step"""
    src = lambda f: open(os.path.join(root, "readtape_amd", "csrc", f)).read()
    sift, api, gain = src("rtfe_sift.hip"), src("rtfe_api.hip"), src("rtfe_gain.hip")
    c = rs.kernel_constants(root)
    c.update(sfs_split="constexpr bool sfs_split(int nt) { return RTFE_SFS_SPLIT && (nt & 1) && nt >= 5; }" in sift and re.search(r"#define RTFE_SFS_SPLIT 1\b", sift) is not None,
             sfs_waves="constexpr int sfs_waves(int nt) { return sfs_split(nt) ? nt / 2 : (nt + 1) / 2; }" in sift,
             sfs_part_strip="constexpr int sfs_part_strip(int nt) { return ((kSfTile + sfs_waves(nt) - 1) / sfs_waves(nt) + 63) / 64; }" in sift,
             sfs_part_rows="constexpr int sfs_part_rows(int nt) { return ((kSfTile + sfs_waves(nt) - 1) / sfs_waves(nt) + sfs_part_strip(nt) - 1) / sfs_part_strip(nt) * sfs_part_strip(nt); }" in sift,
             sfs_last_head="constexpr int H3 = NT - 1, R3 = sfs_part_strip(NT), PR3 = sfs_part_rows(NT), LA3 = PR3 / R3;" in sift,
             ds_warm="int wm = 2 * d.screen[sidx].W + 16; if (wm < 48) wm = 48;" in api,
             es_round="for (int k0 = 0; k0 < n_own; k0 += 64 * kEsAhead) {" in gain and "const int k = k0 + 64 * u + lane;" in gain and re.search(r"#define RTFE_ES_AHEAD 1\b", gain) is not None,
             back="if (back >= 64) { failed = true; why = 7; return 2; }" in gain,
             seg_cut="o.first = i + (long long)sg * SR; o.end = sg + 1 == nseg ? src.iend : i + (long long)(sg + 1) * SR;" in gain)
    return c


def sfs_part(ntrks):
    """(rows of the last head a wave of k_sift_s screens, rows a lane of it screens): sfs_part_rows / sfs_part_strip (rtfe_sift.hip); None where the head is not split"""
    if not ((ntrks & 1) and ntrks >= 5):
        return None
    waves = ntrks // 2
    per = (K_SF_TILE + waves - 1) // waves
    strip = (per + 63) // 64
    return (per + strip - 1) // strip * strip, strip


def ds_warm(W):
    """rows a lane of k_dseg starts in front of its sub-segment (rtfe_api.hip: ds_warm)"""
    return max(2 * W + 16, 48)


def cuts_of(c, W, ntrks, head, prep_run=PREP_RUN, warm=None):
    """the seam classes of the cut between rows c - 1 and c, for a shape on head `head`"""
    out = set()
    hl, hr = sift_halos(W)
    r = c % K_SF_TILE
    if r == 0:
        out.add("sift_tile")
    if r in (K_SF_TILE - hl, hr, K_SF_TILE - W, W + 2):                # (k_sift's halos in front and behind; k_sift_s keeps W rows in front and W + 2 behind)
        out.add("sift_halo")
    if r and r % K_SF_STRIP == 0:
        out.add("sift_strip")
    part = sfs_part(ntrks)
    if part and head == ntrks - 1 and r:
        if r % part[0] == 0:
            out.add("sift_part")
        elif (r % part[0]) % part[1] == 0:
            out.add("sift_pstrip")
    if c % (prep_run * K_SF_TILE) == 0:
        out.add("prep_run")
    if c % K_DS_SUB == 0:
        out.add("dseg_sub")
    if c % K_DS_TILE == 0:
        out.add("dseg_tile")
    if (c + (ds_warm(W) if warm is None else warm)) % K_DS_SUB == 0:
        out.add("dseg_warm")
    return out


def base_tape(kind, seed, noise_mv):
    """(hdr, rows, oracle options) of an unshaped tape: NRZI with one block long enough for four default segments a track and two short ones; GCR and PE as
    fuzz_util.base_tape has them"""
    if kind.startswith("nrzi"):
        n = 7 if kind == "nrzi7" else 9
        spec = synth.nrzi_spec(seed=seed, ntrks=n, noise_mv=noise_mv)
        rng = np.random.default_rng(seed + 2000)
        pay = synth.random_payloads(rng, 1, 30, 50, databits=n - 1) + synth.random_payloads(rng, 1, 1900, 2100, databits=n - 1) + synth.random_payloads(rng, 1, 30, 50, databits=n - 1)
        tape = synth.make_tape(spec, [("block", p) for p in pay], gap_samples=2000)
        opts = (["-ntrks=7"] if n == 7 else []) + (["-m"] if kind.endswith("_m") else [])
    else:
        tape, opts = fuzz_util.base_tape(kind, seed, noise_mv)
    return tape.spec.header(), np.ascontiguousarray(tape.rows), opts


def _extremes(x, amp):
    mid = x[1:-1]
    tops = np.flatnonzero((mid > x[:-2]) & (mid >= x[2:]) & (mid > 0.4 * amp)) + 1
    bots = np.flatnonzero((mid < x[:-2]) & (mid <= x[2:]) & (mid < -0.4 * amp)) + 1
    return np.sort(np.concatenate([tops, bots]))


# ---- the shapes: each writes head t of `rows` around the cut in front of row c, from the extreme at row P (value v, sign s, magnitude mag), and returns the
# first and last row of the shape; rows on both sides of the cut belong to it
def plateau(rows, t, P, c, v, s, mag, W, rng):
    """2 .. W + 2 equal samples at the extreme, across the cut"""
    n = int(rng.integers(2, W + 3))
    a = c - int(rng.integers(1, n))
    lo, hi = min(a, P), max(a + n - 1, P)
    rows[lo:hi + 1, t] = v
    return lo, hi


def double(rows, t, P, c, v, s, mag, W, rng):
    """two tops (bottoms), equal or 1 - 3 codes apart, 2 .. W rows apart, one either side of the cut; between them a hair, a little or a rise threshold lower"""
    k = int(rng.integers(2, W + 1))
    p1 = c - 1 - int(rng.integers(0, k))
    p2 = p1 + k
    delta = int(rng.integers(0, 4))
    u = rng.random()
    frac = rng.uniform(0.0, 0.004) if u < 0.3 else (rng.uniform(0.0, 0.05) if u < 0.6 else rng.uniform(0.03, 0.30))
    lo, hi = min(p1, P), max(p2, P)
    rows[lo:hi + 1, t] = v - s * max(int(round(mag * frac)), delta + 1)
    first = rng.random() < 0.5
    rows[p1, t] = v - s * (0 if first else delta)
    rows[p2, t] = v - s * (delta if first else 0)
    return lo, hi


def valley(rows, t, P, c, v, s, mag, W, rng):
    """a flat top of 2 - 4 samples with a valley of 1 - 3 rows right behind it, deep enough to be the other polarity's candidate; the cut lies inside the flat
    top or between it and the valley"""
    nflat, m = int(rng.integers(2, 5)), int(rng.integers(1, 4))
    e = c - 1 + int(rng.integers(0, nflat - 1))
    lo = min(e - nflat + 1, P)
    rows[lo:e + 1, t] = v
    rows[e + 1:e + m + 1, t] = -s * int(round(mag * rng.uniform(0.3, 1.0)))
    return lo, e + m


def stale(rows, t, P, c, v, s, mag, W, rng):
    """a bottom with a second one 1 - 2 codes different one or two rows behind it: the first lies in front of the cut, the second behind it (the reference's
    window minimum is stale for a row or two; on the device the record's owner lies in the tile in front of its candidate)"""
    gap = int(rng.integers(1, 3))
    p1 = c - 1 - int(rng.integers(0, gap))
    p2 = p1 + gap
    delta = int(rng.integers(1, 3)) * (1 if rng.random() < 0.5 else -1)
    lo, hi = min(p1, P), max(p2, P)
    rows[lo:hi + 1, t] = v - s * (3 + int(rng.integers(0, 3)))
    rows[p1, t] = v
    rows[p2, t] = v + s * delta
    return lo, hi


def notch(rows, t, P, c, v, s, mag, W, rng):
    """a shoulder from the extreme across the cut with a one-row notch at the cut, its depth around the rise threshold"""
    level = v - s * int(round(mag * rng.uniform(0.05, 0.15)))
    depth = max(int(round(mag * rng.uniform(0.03, 0.30))), 2)
    if P < c:
        lo, hi = P, c + int(rng.integers(0, 3))
        rows[P + 1:hi + 1, t] = level
        q = c if P == c - 1 or rng.random() < 0.5 else c - 1
    else:
        lo, hi = c - 1 - int(rng.integers(0, 3)), P
        rows[lo:P, t] = level
        q = c - 1 if P == c or rng.random() < 0.5 else c
    rows[q, t] = level - s * depth
    return lo, hi


def weak(rows, t, P, c, v, s, mag, W, rng):
    """2 - 4 rows above the screen across the cut on a head that is quiet there (P: unused): a run with no sure stretch, what kCrWeak marks"""
    n = int(rng.integers(2, 5))
    a = c - int(rng.integers(1, n))
    h = int(round(mag * rng.uniform(0.03, 0.20)))
    for k in range(n):
        edge = n > 2 and k in (0, n - 1)
        rows[a + k, t] += s * (h // 2 if edge else h - int(rng.integers(0, 3)))
    return a, a + n - 1


WRITERS = {"A-plateau": plateau, "A-double": double, "A-valley": valley, "A-stale": stale, "A-notch": notch, "A-weak": weak}


def shape_rows(hdr, rows0, rng, share=0.25, seg_recs=PK_SEG_RECS):
    """rows0 with the shapes on the row seams inside its blocks and on every peak of a stretch around each multiple of `seg_recs` peaks of a track's block.
    Returns (rows, sites); a site = dict(shape, trk (head), row (its extreme), lo, hi (the shape's rows), cut (the cut it was aimed at, or None))."""
    rows = rows0.astype(np.int64).copy()
    nrows, ntrks = rows.shape
    W = window(hdr)
    busy = np.zeros((nrows, ntrks), bool)
    sites = []
    amps = [int(np.abs(rows0[:, t].astype(np.int64)).max()) for t in range(ntrks)]
    peaks = [_extremes(rows0[:, t].astype(np.int64), amps[t]) for t in range(ntrks)]
    guard = W + 3
    turn = [0]

    def write(shape, t, P, c):
        v = int(rows0[P, t])
        s = 1 if v > 0 else -1
        if shape == "A-weak":
            v, s = 0, (1 if rng.random() < 0.5 else -1)
        if shape == "A-stale" and s > 0:
            return False
        if busy[max(min(P, c) - 2 * guard, 0):max(P, c) + 2 * guard, t].any():
            return False
        lo, hi = WRITERS[shape](rows, t, P, c, v, s, amps[t] if shape == "A-weak" else abs(v), W, rng)
        busy[max(lo - guard, 0):hi + guard + 1, t] = True
        sites.append(dict(shape=shape, trk=int(t), row=int(P), lo=int(lo), hi=int(hi), cut=int(c)))
        return True

    def at_cut(c, heads):
        """the next shape in turn on the head (of `heads`) whose extreme lies nearest the cut; a weak run on a head that is quiet there"""
        for attempt in range(len(SHAPES)):
            shape = SHAPES[turn[0] % len(SHAPES)]
            turn[0] += 1
            cand = []
            for t in heads:
                if shape == "A-weak":
                    if np.abs(rows0[c - W - 4:c + W + 5, t].astype(np.int64)).max() < 0.06 * amps[t]:
                        cand.append((int(rng.integers(0, 100)), t, c))
                elif peaks[t].size:
                    k = int(np.argmin(np.abs(peaks[t] - c)))
                    cand.append((abs(int(peaks[t][k]) - c), t, int(peaks[t][k])))
            cand.sort()
            for d, t, P in cand[:3]:
                if d <= 8 or shape == "A-weak":
                    if write(shape, t, P, c):
                        return True
        return False

    blocks = []
    allp = np.sort(np.concatenate(peaks))
    if allp.size:
        brk = np.flatnonzero(np.diff(allp) > 400)
        blocks = list(zip(np.concatenate([[allp[0]], allp[brk + 1]]), np.concatenate([allp[brk], [allp[-1]]])))
    last = ntrks - 1
    part = sfs_part(ntrks)
    for lo, hi in blocks:
        for c in range(int(lo) + 40 * W, int(hi) - 4 * W):               # (behind the chains' start-up: some twenty peaks in the baseline is fixed)
            cls = cuts_of(c, W, ntrks, last)
            if not cls:
                continue
            rare = cls & {"sift_tile", "sift_halo", "prep_run", "dseg_tile", "sift_part"}
            if not rare and rng.random() >= share * (0.1 if cls <= {"sift_pstrip"} else 0.5):      # (the 4-, 14-, 128-row grids are dense: a share of their cuts will do)
                continue
            # the last head is split four (three) ways in k_sift_s: its cuts are its own; every other cut takes the last head every other time
            if cls <= {"sift_part", "sift_pstrip"}:
                at_cut(c, [last])
            else:
                if rare and part:
                    at_cut(c, [last])
                at_cut(c, list(range(ntrks - 1)) if rng.random() < 0.6 else list(range(ntrks)))
    # the cuts counted in records: every peak of a stretch around each multiple of seg_recs peaks of a track's block gets a shape, whichever record the count began at
    # (the shape's own cut: right behind its extreme, or where the next row seam lies if that is nearer than a window)
    for t in range(ntrks):
        pk = peaks[t]
        if pk.size < 2 * seg_recs:
            continue
        starts = np.concatenate([[0], np.flatnonzero(np.diff(pk) > 400) + 1, [pk.size]])
        for a, b in zip(starts[:-1], starts[1:]):
            for j in range(1, (b - a) // seg_recs + 1):
                for P in pk[a + j * seg_recs - 8:min(a + j * seg_recs + 40, b - 2)]:
                    shape = SHAPES[turn[0] % (len(SHAPES) - 1)]          # (no weak run here: it needs a quiet head, not a peak)
                    turn[0] += 1
                    if write(shape, t, int(P), int(P) + 1):
                        sites[-1]["cut"] = None
    out = np.clip(rows, -32767, 32767)
    return np.ascontiguousarray(out.astype(np.int16)), sites


def coverage(sites, hdr, prep_run=PREP_RUN, warm=None):
    """{class: count}: the sites per shape class, and per row-seam class the sites whose rows lie on both sides of a cut of that class"""
    W = window(hdr)
    cnt = {}
    for s in sites:
        cnt[s["shape"]] = cnt.get(s["shape"], 0) + 1
        on = set()
        for c in range(s["lo"] + 1, s["hi"] + 1):
            on |= cuts_of(c, W, hdr.ntrks, s["trk"], prep_run, warm)
        if s["shape"] == "A-stale" and any("sift_tile" in cuts_of(c, W, hdr.ntrks, s["trk"]) for c in range(s["lo"] - K_PK_BACK + 1, s["lo"] + 1)):
            on.add("back_tile")                                          # (the bottom's forced-rescan look-back of kPkBack rows starts behind the tile's front edge)
        for k in on:
            cnt[k] = cnt.get(k, 0) + 1
        if s["trk"] == hdr.ntrks - 1:
            cnt["last_head"] = cnt.get("last_head", 0) + 1
    return cnt


def draw(seed):
    """the parameters of tape `seed` (one place: the tool and the tests draw the same tapes)"""
    rng = np.random.default_rng(seed + 17_000_000)
    return dict(kind=str(rng.choice(KINDS)), noise_mv=float(rng.choice([2.0, 5.0, 10.0])), share=float(rng.choice([0.15, 0.25, 0.4])))


def shaped(seed, **over):
    """(hdr, unshaped rows, shaped rows, sites, oracle options) of tape `seed`"""
    d = dict(draw(seed), **over)
    hdr, rows0, opts = base_tape(d["kind"], seed, d["noise_mv"])
    rows, sites = shape_rows(hdr, rows0, np.random.default_rng(seed * 7919 + 31), share=d["share"])
    assert not (rows == -32768).any()
    return hdr, rows0, rows, sites, opts


def phased(rows, k):
    """the tape with k quiet rows in front: every shape moves against every row grid at once, and no shape changes"""
    return np.ascontiguousarray(np.concatenate([np.zeros((k, rows.shape[1]), rows.dtype), rows]))


def phase_sites(sites, k):
    return [dict(s, row=s["row"] + k, lo=s["lo"] + k, hi=s["hi"] + k, cut=None if s["cut"] is None else s["cut"] + k) for s in sites]


def seg_counts(err):
    """the counts of the emulator's seg_shapes: lines in `err` (one line a scan of the peak path under RTFE_PREP_CHECK=2), summed; and the number of lines"""
    tot, n = dict.fromkeys(SEG_COUNTS, 0), 0
    for line in err.splitlines():
        if line.startswith("seg_shapes:"):
            w = line.split()
            kv = dict(zip(w[1::2], w[2::2]))
            for k in SEG_COUNTS:
                tot[k] += int(kv[k])
            n += 1
    return tot, n


def fast(st):
    """did the fast paths take the tape: nothing redone, no chain gave up, and the lean step took more than twice what the general step took"""
    return st["redone"] == 0 and not any(st["gave_up"]) and st["parallel"] > 2 * st["sequential"]
