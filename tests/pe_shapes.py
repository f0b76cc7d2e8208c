"""PE tapes aimed at where a track's preamble ends: the inputs of tests/test_emul_pe_shapes.py, tests/test_gpu_pe_shapes.py and tools/fuzz_shapes.py --pe.
Test infrastructure.

The device mirrors pe_preamble_peak (src/decode_pe.c:127-155) so that the AGC state it reads back is the block decoder's: peaks 5 .. 15 with v_top > v_bot
are learned, and the first peak with peakcount > 70, the polarity of a one and t_peak - t_lastpeak > t_clkwindow flips `datablock` (agc_after_peak_m in
rtfe_kernels.hip, used by k_decode and k_dchain's fire(); the general step of k_gain; and the gate `!datablock && peakcount >= 68` that decides whether a
peak's time is computed at all).  Every other PE tape of the suite has a 40-bit preamble, no tape mark, clk_factor 1.4 or 1.5 and an undamaged preamble: the
count passes 70 nine peaks in front of the marker and the marker's interval is a quarter of a bit clear of the window.  The classes here leave that case:

  P-length  preambles (and postambles) of 20, 33, 34, 35, 36, 37, 40 and 90 zero bits: a clean preamble of n zeros has 2n - 1 peaks and the marker is
            peak 2n - so 36 is the shortest the reference reads (peak 72), 35 misses by one, and with 20 the switch falls inside the data or never
  P-mark    PE tape marks of 60, 72 and 90 flux changes between and behind blocks: the count passes 70 with no one in sight
  P-drop    a stretch of several tracks' preambles attenuated to 2 .. 30 %: over peaks 60 .. 76 (the count lags: the marker arrives at 70 or less), over
            peaks 4 .. 16 (the whole learning range 5 .. 15 and the peak on each side), over the marker itself.  The tape's own amplitude is 0.6 V, so that the lower third of that range falls below the rise threshold of
            a fresh detector (0.1 V) and is not counted, and the rest is counted and learned at its small height.  A dropout that multiplies cannot
            put a top under a bottom, so every counted peak 5 .. 15 is learned: over peaks 4 .. 16 either the count lags and full-size peaks are learned,
            or small heights are (`height` well under the tape's); drop_hits() says per site which, and a site that is neither fails its test.  Every track that reaches the switch has learned at least one height; none at all is
            0 / 0, the reference's fatal "avg peak-to-peak voltage isn't positive" exit, which tests/cases.py's nrzi9_avgheight_fatal pins and which is
            left out here
  P-clk     parameter sets whose t_clkwindow - evaluated in float32 exactly as rtfe_api.hip does - is the largest float32 below, the float32 nearest to (or equal to) and
            the smallest float32 above the smallest and the largest interval in front of a candidate peak, as the oracle at clk_factor 1.5 measured them: the
            half-bit intervals of the preamble's peaks past 70 (ladder "half") and the one-bit intervals in front of the markers (ladder "one"); plus 2.0
            (the range's end in rt_parmsets.c) and a set one float32 ulp of clk_factor away from another.  Up to eight sets a scan (a .parms file for the
            oracle, FrontEndConfig.parmsets for the front end): the dense path's de-duplication has to keep sets apart whose windows differ by one ulp.
            The blocks carry a parity error so that the reference tries every set.
            Equality (what pins `>` against `>=`): an interval is the difference of two doubles, each a double row time minus a float32 product
            widened to double; t_clkwindow is a float32.  Under the suite's usual tstart_ns of 1 ms the row times carry bits far below a float32's
            and no interval is a float32 (float32_intervals() counts them: none).  The generator DOES reach equality by starting the tape at
            tstart_ns = 3e12: a time between 2048 s and 4096 s is a multiple of 2^-41 s in double, so every interval is one too, and between 2^-18 s
            and 2^-17 s (3.8 .. 7.6 us: the half-bit intervals at 1600 bpi, 50 ips) that is exactly a float32's spacing, and twice as fine as one
            between 2^-17 s and 2^-16 s (the one-bit intervals: every other multiple is a float32).  The ladder then holds the interval's own value
            between its two neighbours, and classes_met counts the candidates that sit on their window (`equal`).
  P-jit     jitter 0.08 .. 0.15 of a bit cell: the intervals spread round the window at the stock factors 1.4 and 1.5 (-m)
  P-shape   seam_shapes' plateau, double, notch and valley on the marker peak and on the peak in front of it (they move left_distance and the half-sample
            code, and so t_peak by half samples), and on peaks 1, 5, 15, 16, 69, 70 and 71 of a track
  P-seam    the gap in front of a block chosen so that a cut of k_dseg (dseg_sub, dseg_tile, dseg_warm of seam_shapes.cuts_of) lies between the marker
            peak's row and its detection: the record-to-literal join of k_dchain and its flip to the lean step meet the switch
  P-time    the rows of a P-length tape under headers with tstart_ns 0 and 3e12: time_of's double arithmetic and the bits of t_peak

-invert and a -skew= list are options of every class (tape(..., invert=, skew=)).  Tapes are 9-track PE, one to five blocks of 40 .. 80 bytes, at most
25 000 rows, deterministic per seed.  classes_met() says from the oracle's dump alone what a tape contains; a test asserts it before it asserts parity."""
import os
import re

import numpy as np

import seam_shapes as ss
from rail_shapes import K_DS_SUB, K_DS_TILE, window
from readtape_amd import frontend, synth

CLASSES = ("P-length", "P-mark", "P-drop", "P-clk", "P-jit", "P-shape", "P-seam", "P-time")
LENGTHS = (20, 33, 34, 35, 36, 37, 40, 90)
MARK_FLUX = (60, 72, 90)
PRE_COUNT, LEARN_FIRST, LEARN_LAST, TIME_GATE = 70, 5, 15, 68      # mirrored from the kernels: kernel_constants()
SHAPE_PEAKS = (1, 5, 15, 16, 69, 70, 71)
SHAPES = ("A-plateau", "A-double", "A-notch", "A-valley")
SEAM_CUTS = ("dseg_sub", "dseg_tile", "dseg_warm")
SKEW = "-skew=3,1,2,0,3,0,1,2,1"
MAX_ROWS = 25000
GAP = 900
CLK_TSTART = 3_000_000_000_000                                         # ns, P-clk: fifty minutes into a recording (see the class's note on equality)
DROP_AMPLITUDE = 0.6                                                   # volts, P-drop: some 1 V from top to bottom, so that under a tenth of it a peak falls below the start-up rise of 0.1 V
LEAD = 8.0                                                             # cells of lead-in synth._render_block puts in front of a block
PARMS_HEAD = "parms active, clk_window, clk_alpha, agc_window, agc_alpha, min_peak, clk_factor, pulse_adj, pkww_bitfrac, pkww_rise, midbit, z1pt, z2pt, id\n"


def kernel_constants(root):
    """what the generator mirrors from the sources: the count, the learning range, the three time gates, the expression of t_clkwindow, the condition of the
    de-duplication, the expression of the peak time.  A retune fails tests/test_emul_pe_shapes.py instead of un-aiming the tapes."""
    src = lambda f: open(os.path.join(root, "readtape_amd", "csrc", f)).read()
    ker, dense, gain, api = src("rtfe_kernels.hip"), src("rtfe_dense.hip"), src("rtfe_gain.hip"), src("rtfe_api.hip")
    m = re.search(r"if \(w\.peakcount > (\d+) && w\.bit1_up == is_top && t_peak - w\.t_lastpeak > P\.t_clkwindow\) \{", ker)
    l = re.search(r"else if \(w\.peakcount >= (\d+) && w\.peakcount <= (\d+) && w\.v_top > w\.v_bot\) \{", ker)
    g = [re.search(r"const bool need_time = cfg->mode == RTFE_PE && !w\.datablock && w\.peakcount >= (\d+);", ker),
         re.search(r"if \(cmode == RTFE_PE && !w\.datablock && w\.peakcount >= (\d+)\) \{", dense),
         re.search(r"if \(cmode == RTFE_PE && !w\.datablock && w\.peakcount >= (\d+)\) \{", gain)]
    tp = "- ((float)(W - ld) - adj) * cfg.sample_deltat;"
    return dict(pre_count=int(m.group(1)) if m else None,
                learn=(int(l.group(1)), int(l.group(2))) if l else None,
                gates=tuple(int(x.group(1)) if x else None for x in g),
                clkwindow="const float bitspace = density_mode ? 0.0f : 1 / (c->bpi * c->ips);" in api and "dp.t_clkwindow = bitspace / 2 * ps.clk_factor;" in api,
                dedup=("if (a.W == b.W && a.rise == b.rise && a.min_peak == b.min_peak && a.agc_alpha == b.agc_alpha && a.agc_window == b.agc_window\n"
                       "                && (c->mode != RTFE_PE || a.t_clkwindow == b.t_clkwindow)) break; }") in api,
                t_peak=tp in dense and tp in gain and "- ((float)(P.W - left_distance) - adj) * cfg->sample_deltat;" in ker
                and "return (double)(c->tstart_ns + abs_row * c->tdelta_ns) / 1e9; }" in ker,
                cf_range="PD(clk_factor, 0, 0, 2)" in open(os.path.join(root, "readtape_amd", "csrc", "host", "rt_parmsets.c")).read())


# ---- t_clkwindow in float32, as rtfe_api.hip forms it
def half_bit(hdr):
    return np.float32(np.float32(1) / (np.float32(hdr.bpi) * np.float32(hdr.ips or 50.0))) / np.float32(2)


def clkwindow(hdr, cf):
    return np.float32(half_bit(hdr) * np.float32(cf))


def cf_for(hdr, target):
    """a float32 clk_factor whose t_clkwindow is the float32 `target` (None where no factor gives it)"""
    target = np.float32(target)
    cf = np.float32(target / half_bit(hdr))
    for _ in range(4):
        for c in (cf, np.nextafter(cf, np.float32(0)), np.nextafter(cf, np.float32(4))):
            if clkwindow(hdr, c) == target:
                return np.float32(c)
        cf = np.nextafter(cf, np.float32(4)) if clkwindow(hdr, cf) < target else np.nextafter(cf, np.float32(0))
    return None


def parmset(cf):
    """the reference's first PE set (src/parmsets.c) with another clk_factor, as the front end sees it"""
    return (0.7, 0.10, 0.0, 0.0, 5, float(np.float32(cf)))


def parms_text(cfs):
    return PARMS_HEAD + "".join(f"{{1, 0, 0.2, 5, 0.0, 0.0, {np.float32(cf):.9g}, 0.4, 0.7, 0.1, 0.5, 1.45, 2.35, PRM}}\n" for cf in cfs)


# ---- the tapes
def encode(payload, pre, post, bad_parity=False, ntrks=9):
    """synth.pe_encode with the lengths given; bad_parity: the parity bit of the middle byte is wrong (the reference then tries every parameter set)"""
    if not bad_parity:
        return synth.pe_encode(payload, ntrks, pre=pre, post=post)
    per, signs = [], []
    words = [((b << 1) | (synth._parity9(b) ^ 1)) for b in payload]
    words[len(words) // 2] ^= 1
    for t in range(ntrks):
        bits = np.asarray([0] * pre + [1] + [(w >> (ntrks - 1 - t)) & 1 for w in words] + [1] + [0] * post, dtype=np.int64)
        p, s = synth._pe_track_transitions(bits)
        per.append(p); signs.append(s)
    return per, float(pre + 1 + len(payload) + 1 + post), signs


def _build(seed, blocks, noise_mv=10.0, jitter=0.02, tstart_ns=1_000_000, gaps=None, amplitude=2.5):
    """blocks: dicts(pre, post, n (bytes), bad) or dict(mark=nflux).  gaps: extra quiet rows in front of item i.  Returns (tape, meta): per item its first
    row, its per-track transition cells and what it was made of."""
    spec = synth.pe_spec(seed=seed, noise_mv=noise_mv, jitter=jitter, tstart_ns=tstart_ns, amplitude=amplitude)
    rng = np.random.default_rng(seed + 2000)
    items, meta = [], []
    for i, b in enumerate(blocks):
        if gaps and gaps.get(i):
            items.append(("gap", int(gaps[i])))
        if "mark" in b:
            cells, ncells, signs = synth.pe_tapemark(9, b["mark"])
        else:
            pay = bytes(rng.integers(0, 256, size=b["n"], dtype=np.int64).astype(np.uint8))
            cells, ncells, signs = encode(pay, b["pre"], b["post"], b.get("bad", False))
        items.append(("raw", cells, ncells, signs))
        meta.append(dict(b, cells=cells))
    tape = synth.make_tape(spec, items, gap_samples=GAP)
    for m, blk in zip(meta, tape.blocks):
        m["start"], m["end"] = blk[1], blk[2]
    assert tape.rows.shape[0] <= MAX_ROWS, tape.rows.shape
    return tape, meta


def block_rows(spec, b):
    """rows synth._render_block gives the item"""
    ncells = b["mark"] // 2 if "mark" in b else b["pre"] + 1 + b["n"] + 1 + b["post"]
    return int(np.ceil((ncells + 2 * LEAD) * spec.samples_per_bit))


def peak_row(rows, spb, m, t, k):
    """the row of the extreme of peak k (1 = the first) of track t of item m: the sample nearest the transition's centre, moved to the local extreme"""
    c = int(round(m["start"] + (LEAD + m["cells"][t][k - 1] + 0.5) * spb))
    x = rows[c - 3:c + 4, t].astype(np.int64)
    return c - 3 + int(np.argmax(np.abs(x)))


def marker_peak(m):
    """the number of the marker peak on a clean tape: n zeros are n data and n - 1 phase transitions"""
    return 2 * m["pre"]


def _lengths(seed, nblocks):
    rng = np.random.default_rng(seed + 41_000_000)
    pres = [LENGTHS[(seed * nblocks + i) % len(LENGTHS)] for i in range(nblocks)]
    posts = [int(x) for x in rng.choice(LENGTHS[:7], nblocks)]                          # (a 90-bit postamble beside a 90-bit preamble would outgrow 25 000 rows)
    return [dict(pre=p, post=q, n=int(rng.integers(40, 81))) for p, q in zip(pres, posts)]


def tape(cls, seed, invert=False, skew=False, m=False, **over):
    """tape `seed` of class `cls`: dict(hdr, rows, rows0 (before a dropout or a shape was written), opts (the oracle's, -parms= apart), parmsets (None: the defaults), parms_text, meta, sites, spb)"""
    assert cls in CLASSES, cls
    rng = np.random.default_rng(seed * 7919 + 57)
    sites, sets, text = [], None, None
    if cls in ("P-length", "P-time"):
        blocks = _lengths(seed, 4)
        if over.get("pres"):                                                                # (tests/cases.py: a golden of its own per length)
            blocks = [dict(pre=p, post=40, n=int(rng.integers(40, 61))) for p in over["pres"]]
        t, meta = _build(seed, blocks, tstart_ns=over.get("tstart_ns", 1_000_000))
        rows = t.rows
    elif cls == "P-mark":
        fl = [MARK_FLUX[(seed + i) % 3] for i in range(3)]
        t, meta = _build(seed, [dict(pre=40, post=40, n=int(rng.integers(40, 81))), dict(mark=fl[0]), dict(pre=36, post=40, n=int(rng.integers(40, 81))), dict(mark=fl[1]), dict(mark=fl[2])][:over.get("nitems", 5)])
        rows = t.rows
    elif cls == "P-jit":
        t, meta = _build(seed, [dict(pre=p, post=40, n=int(rng.integers(40, 81))) for p in (40, 36, 37, 40)], jitter=float(over.get("jitter", rng.uniform(0.08, 0.15))))
        rows = t.rows
    elif cls == "P-clk":
        t, meta = _build(seed, [dict(pre=p, post=40, n=int(rng.integers(40, 61)), bad=True) for p in (40, 36, 37)[:over.get("nblocks", 3)]],
                         tstart_ns=over.get("tstart_ns", CLK_TSTART))
        rows = t.rows
    elif cls == "P-drop":
        t, meta = _build(seed, [dict(pre=p, post=40, n=int(rng.integers(40, 81))) for p in (40, 37, 40, 38)[:over.get("nblocks", 4)]], noise_mv=3.0, amplitude=DROP_AMPLITUDE)
        rows = t.rows.astype(np.float64)
        spb = t.spec.samples_per_bit
        for i, b in enumerate(meta):
            place = ("count", "learn", "marker", "count")[(i + seed) % 4]
            a, z = {"count": (60, 76), "learn": (LEARN_FIRST - 1, LEARN_LAST + 1), "marker": (marker_peak(b) - 1, marker_peak(b) + 1)}[place]
            for trk in sorted(int(x) for x in rng.choice(9, int(rng.integers(2, 6)), replace=False)):
                a1 = a + int(rng.integers(0, 3)) if place == "count" else a            # (the learning range and the marker are covered whole, with the peak on each side)
                z1 = z - int(rng.integers(0, 3)) if place == "count" else z
                lo = int(b["start"] + (LEAD + b["cells"][trk][a1 - 1] + 0.25) * spb)
                hi = int(b["start"] + (LEAD + b["cells"][trk][z1 - 1] + 0.75) * spb)
                f = float(np.exp(rng.uniform(np.log(0.02), np.log(0.30))))
                rows[lo:hi + 1, trk] *= f
                sites.append(dict(place=place, block=i, trk=trk, lo=lo, hi=hi, factor=f, peaks=(a1, z1)))
        rows = np.rint(rows).astype(np.int16)
    elif cls == "P-shape":
        t, meta = _build(seed, [dict(pre=p, post=40, n=int(rng.integers(40, 81))) for p in (40, 36, 37, 40)], noise_mv=5.0)
        rows = t.rows.astype(np.int64)
        spb, W = t.spec.samples_per_bit, window(t.spec.header())
        turn = seed
        for i, b in enumerate(meta):
            trks = [int(x) for x in rng.permutation(9)]
            todo = [(trk, marker_peak(b) - (j & 1)) for j, trk in enumerate(trks[:6])] + [(trks[6 + j % 3], k) for j, k in enumerate(SHAPE_PEAKS)]
            for trk, k in todo:
                P = peak_row(t.rows, spb, b, trk, k)
                v = int(t.rows[P, trk]); s = 1 if v > 0 else -1
                shape = SHAPES[turn % len(SHAPES)]; turn += 1
                lo, hi = ss.WRITERS[shape](rows, trk, P, P + int(rng.integers(0, 2)), v, s, abs(v), W, rng)
                sites.append(dict(shape=shape, block=i, trk=trk, peak=k, row=P, lo=int(lo), hi=int(hi), marker=k >= marker_peak(b) - 1))
        rows = np.clip(rows, -32767, 32767).astype(np.int16)
    elif cls == "P-seam":
        blocks = [dict(pre=p, post=40, n=int(rng.integers(40, 61))) for p in (40, 36, 37, 40, 36)]
        spec = synth.pe_spec(seed=seed)
        spb, W = spec.samples_per_bit, window(spec.header())
        pos, gaps = GAP, {}
        for i, b in enumerate(blocks):
            cut = SEAM_CUTS[(i + seed) % 3]
            off = int(round((LEAD + (b["pre"] + 0.5)) * spb))                              # the marker: the data transition of cell `pre`
            aim = pos + off + (0, W // 2, W + 1)[(i // 3 + seed) % 3]                       # the cut at the marker's row, half-way, or at its detection
            grid, ph = {"dseg_sub": (K_DS_SUB, 0), "dseg_tile": (K_DS_TILE, 0), "dseg_warm": (K_DS_SUB, -ss.ds_warm(W))}[cut]
            extra = (ph - aim) % grid
            gaps[i] = extra
            sites.append(dict(block=i, cut=cut, row=aim + extra))
            pos += extra + block_rows(spec, b) + GAP
        t, meta = _build(seed, blocks, gaps=gaps)
        rows = t.rows
    hdr = t.spec.header()
    opts = (["-invert"] if invert else []) + ([SKEW] if skew else []) + (["-m"] if m or cls in ("P-jit", "P-clk") else [])
    rows = np.ascontiguousarray(rows)
    assert rows.dtype == np.int16 and not (rows == -32768).any() and rows.shape[0] <= MAX_ROWS
    import dataclasses
    return dict(cls=cls, seed=seed, tape=dataclasses.replace(t, rows=rows), hdr=hdr, rows=rows, rows0=np.ascontiguousarray(t.rows), opts=opts, parmsets=sets, parms_text=text, meta=meta, sites=sites, spb=t.spec.samples_per_bit)


def with_ladder(tp, cfs):
    """the tape under the parameter sets of a clk_factor ladder"""
    return dict(tp, parmsets=[parmset(c) for c in cfs], parms_text=parms_text(cfs), opts=[o for o in tp["opts"] if o != "-m"] + ["-m"])


def config(tp, **kw):
    """the front end's configuration of a tape: the default sets (eight under -m) or the tape's own"""
    opts = tp["opts"]
    sets = tp["parmsets"] or frontend.DEFAULT_PARMSETS[frontend.PE][:8 if "-m" in opts else 1]
    skew = next(([int(x) for x in o[6:].split(",")] for o in opts if o.startswith("-skew=")), None)
    return frontend.FrontEndConfig.from_header(tp["hdr"], parmsets=sets, skew=skew, invert="-invert" in opts, **kw)


def oracle_opts(tp, wd):
    """the oracle's options; a tape with sets of its own gets its .parms file written into wd"""
    if not tp["parms_text"]:
        return list(tp["opts"])
    path = os.path.join(wd, "pe_shapes.parms")
    with open(path, "w") as f:
        f.write(tp["parms_text"])
    return list(tp["opts"]) + [f"-parms={path}"]


# ---- what a tape contains, from the oracle's dump alone
def _track_view(hdr, e, t, window_t):
    x = e[e["trk"] == t]
    if x.size == 0:
        return None
    pc, h, tp, top = x["peakcount"], x["v_avg_height"], x["t_peak"], x["kind"] == 0
    ch = np.flatnonzero(h != np.float32(4.0))
    # the dump is written in front of the block decoder's callback: the first record whose v_avg_height is not 4.0 is the peak BEHIND the switch
    sw = int(ch[0]) - 1 if ch.size else None
    iv = np.diff(tp, prepend=tp[0])
    bit = 2.0 * float(half_bit(hdr))
    full = np.flatnonzero((iv > 0.75 * bit) & (np.arange(x.size) >= 2))
    mk = int(full[0]) if full.size else None                              # the first interval of a whole bit: the marker, on a clean tape
    end = sw if sw is not None else x.size - 1
    # heights learned: peaks 5 .. 15 in front of the switch whose last top lies above the last bottom
    vt = vb = 0.0
    heights = []
    for k in range(min(end + 1, x.size)):
        if top[k]: vt = float(x["v_peak"][k])
        else: vb = float(x["v_peak"][k])
        if LEARN_FIRST <= pc[k] <= LEARN_LAST and vt > vb and k != sw:
            heights.append(vt - vb)
    learned = len(heights)
    one_is_top = not top[0]                                                # bit1_up = !is_top of the first peak
    cand = np.flatnonzero((pc > PRE_COUNT) & (top == one_is_top) & (np.arange(x.size) <= end) & (np.arange(x.size) >= 1))
    margin = float(np.abs(iv[cand] - float(window_t)).min() / (hdr.tdelta_ns * 1e-9 / 2)) if cand.size else None
    where = "never" if sw is None else ("data" if mk is not None and sw > mk else ("71-72" if int(pc[sw]) in (PRE_COUNT + 1, PRE_COUNT + 2) else "later"))
    return dict(trk=t, switch=None if sw is None else int(pc[sw]), where=where, learned=learned, margin=margin, candidates=int(cand.size),
                height=float(h[ch[0]]) if ch.size else None, peaks=int(pc[-1]), learned_heights=heights,
                marker_t=None if mk is None else float(tp[mk]),
                marker_count=None if mk is None else int(pc[mk]),
                cand_intervals=iv[cand], cand_at_switch=None if sw is None else float(iv[sw]))


def classes_met(hdr, attempts, windows=None):
    """per attempt and track: the peakcount at which v_avg_height first leaves 4.0 (`switch`; None: never); `where` it fell ("71-72", "later": at a later
    count but still at the first whole-bit interval, "data": behind it, "never"); how many heights were `learned` and the `height` the switch set; the smallest |interval - t_clkwindow| at a
    candidate (count > 70, the polarity of a one) in half samples (`margin`).  windows: t_clkwindow per parameter set (default: the stock sets')."""
    if windows is None:
        windows = [clkwindow(hdr, p[5]) for p in frontend.DEFAULT_PARMSETS[frontend.PE]]
    out = []
    for a in attempts:
        for t in range(hdr.ntrks):
            v = _track_view(hdr, a["events"], t, windows[a["parmset"]])
            if v is not None:
                out.append(dict(v, attempt=a["start"], parmset=a["parmset"]))
    return out


def totals(met):
    """the counters the tests assert and the fuzzer prints"""
    c = dict(tracks=len(met), sw_71_72=0, sw_later=0, sw_data=0, sw_never=0, learned_small=0, learned_min=99, height_low=0, never_past70=0, marker_le70=0, near_1=0, near_4=0, equal=0)
    hs = [v["height"] for v in met if v["height"] is not None]
    typical = float(np.median(hs)) if hs else 0.0
    for v in met:
        c["sw_" + v["where"].replace("-", "_")] += 1
        c["learned_small"] += bool(v["learned_heights"]) and min(v["learned_heights"]) < 0.5 * typical      # a height under half the tape's was learned
        if v["switch"] is not None:
            c["learned_min"] = min(c["learned_min"], v["learned"])
        c["height_low"] += v["height"] is not None and v["height"] < 0.6 * typical
        c["never_past70"] += v["switch"] is None and v["peaks"] > PRE_COUNT
        c["marker_le70"] += v["marker_count"] is not None and v["marker_count"] <= PRE_COUNT
        if v["margin"] is not None:
            c["near_1"] += v["margin"] < 1.0
            c["near_4"] += v["margin"] < 4.0
            c["equal"] += v["margin"] == 0.0
    return c


def ladders(hdr, attempts):
    """the clk_factor ladders of P-clk from the oracle's run at clk_factor 1.5 (`attempts` of parameter set 0): {"half": [...], "one": [...], "both": [...]}, up to eight
    float32 factors each - below / nearest / above the smallest and the largest interval, 2.0, and one factor an ulp above another."""
    half, one = [], []
    w15 = clkwindow(hdr, 1.5)
    for v in classes_met(hdr, [a for a in attempts if a["parmset"] == 0], [w15] * 8):
        iv = v["cand_intervals"]
        half += [float(x) for x in iv[iv <= float(w15)]]
        one += [float(x) for x in iv[iv > float(w15)]]
    out = {}
    for name, ivs in (("half", half), ("one", one)):
        cfs = []
        uniq = sorted({float(np.float32(x)): x for x in sorted(ivs)}.values())             # one interval per float32 value
        for target in [uniq[0], uniq[-1]] + ([uniq[len(uniq) // 2]] if len(uniq) > 2 else []):
            near = np.float32(target)
            lo = near if float(near) < target else np.nextafter(near, np.float32(0))      # the largest float32 below the interval
            hi = np.nextafter(near if float(near) == target else lo, np.float32(1))        # the smallest above
            for w in (lo, near, hi):                                                        # (the nearest: the interval itself where it is a float32, else one of the two)
                cf = cf_for(hdr, w)
                if cf is not None and 0 <= cf <= 2 and not any(cf == c for c in cfs):
                    cfs.append(cf)
        cfs = cfs[:6]
        if not any(c == np.float32(2.0) for c in cfs):
            cfs.append(np.float32(2.0))
        up = np.nextafter(cfs[0], np.float32(4))                                            # one float32 ulp of clk_factor above the first
        if not any(c == up for c in cfs):
            cfs.append(up)
        out[name] = cfs[:8]
    both = []
    for c in out["half"][:5] + out["one"][:2] + [np.float32(2.0)]:                          # eight sets of one scan: both thresholds and the range's end
        if not any(c == x for x in both):
            both.append(c)
    out["both"] = both
    return out


def drop_hits(tp, attempts):
    """P-drop: what the oracle's dump says of the (attempt, track) pairs the generator's sites lie in, per placement.  `learn`: the tracks (`n`), those that
    learned a height under half the tape's typical one (`small`: the stretch was counted and learned at its small size) and those whose marker came at a
    count under the clean tape's 2 * pre (`lag`: peaks of the stretch fell below the rise and were not counted, so later, full-size peaks were peaks 5 .. 15);
    `miss`: neither - the dropout changed nothing the preamble's logic reads.  `count`: `n`, and `lag` as above.  `marker`: `n`, and `moved`: the switch
    not at the clean tape's count 2 * pre."""
    views = []
    for a in attempts:
        for t in range(tp["hdr"].ntrks):
            v = _track_view(tp["hdr"], a["events"], t, clkwindow(tp["hdr"], 1.5))
            if v is not None:
                views.append((a, t, v))
    hs = [h for _, _, v in views for h in v["learned_heights"]]
    typical = float(np.median(hs)) if hs else 0.0
    out = {p: dict(n=0, small=0, lag=0, miss=0, moved=0) for p in ("learn", "count", "marker")}
    for s in tp["sites"]:
        clean = marker_peak(tp["meta"][s["block"]])
        for a, t, v in views:
            if t != s["trk"] or not a["start"] <= s["lo"] < a["end"]:
                continue
            c = out[s["place"]]
            small = bool(v["learned_heights"]) and min(v["learned_heights"]) < 0.5 * typical
            lag = v["marker_count"] is not None and v["marker_count"] < clean
            c["n"] += 1; c["small"] += small; c["lag"] += lag; c["miss"] += not (small or lag); c["moved"] += v["switch"] != clean
    return out


def float32_intervals(met):
    """how many candidate intervals are float32 values themselves (only those can equal a t_clkwindow)"""
    return sum(int((v["cand_intervals"] == v["cand_intervals"].astype(np.float32).astype(np.float64)).sum()) for v in met)


def seam_hits(hdr, met):
    """P-seam, from the oracle's dump: per cut class, the (marker row, track) pairs whose marker peak - the peak behind the first whole-bit interval, its row
    taken from its t_peak - has a cut of that class between the row in front of its extreme and its detection"""
    W = window(hdr)
    seen, cnt = set(), {}
    for v in met:
        if v["marker_t"] is None:
            continue
        r = int(round((v["marker_t"] * 1e9 - hdr.tstart_ns) / hdr.tdelta_ns))
        if (r, v["trk"]) in seen:                                             # (-m: a block's attempts see the same marker)
            continue
        seen.add((r, v["trk"]))
        on = set()
        for c in range(r, r + W + 3):
            on |= ss.cuts_of(c, W, hdr.ntrks, v["trk"]) & set(SEAM_CUTS)
        for k in on:
            cnt[k] = cnt.get(k, 0) + 1
    return cnt


def draw(seed):
    """the parameters of fuzz tape `seed` (tools/fuzz_shapes.py --pe)"""
    rng = np.random.default_rng(seed + 23_000_000)
    cls = str(rng.choice([c for c in CLASSES]))
    return dict(cls=cls, invert=bool(rng.random() < 0.3), skew=bool(rng.random() < 0.25), m=bool(rng.random() < 0.4),
                path=str(rng.choice(["dense", "dense", "decode", "peak", "peak_slow", "lean0"])))


PATHS = {"dense": {}, "decode": {"RTFE_DENSE_PATH": "0"}, "peak": {"RTFE_PEAK_PATH": "1"}, "peak_slow": {"RTFE_PEAK_PATH": "1", "RTFE_GAIN_FAST": "0"}, "lean0": {"RTFE_DS_LEAN": "0"}}
