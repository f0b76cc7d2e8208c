"""The int16 rails written onto short clean tapes for the amplitude (peak) detectors: the inputs of tools/fuzz_shapes.py --rails and of tests/test_*_rails.py.
Test infrastructure.

A digitiser that clips delivers plateaus at -32768 and 32767.  -32768 is a sample like any other, and -invert turns it into +32768 (the reference negates the
VOLTAGE, src/readtape.c:1420-1421), a code no int16 holds - while records, margins, packed lanes and LDS tiles on the device are 16 bits wide.  The tapes
here put that code where the kernels cut the tape: the first and last rows of a k_sift tile and of its halos, the rows where a run of k_prep's tiles ends,
k_gain_seg's segments (counted in a track's peaks), k_dseg's sub-segments and tiles, k_decode's 64-row groups and tiles.  Shapes: the whole tape multiplied
and clipped (every excursion a plateau); single -32768 bottoms and 32767 tops; plateaus of -32767 with one -32768 first, in the middle or last (under
-invert the unique extreme of its window); 32767 next to -32768 (65 535 codes between adjacent rows); a lone -32768 in an inter-block gap; the tape's first
and last row; the rows inside a skewed track's deskew delay.  Column 0 never holds -32768: there it is the TBIN end mark.  Deterministic per seed."""
import dataclasses
import os
import re

import numpy as np

from readtape_amd import frontend, synth, tbin

# the seams, mirrored from the kernels (test_emul_rails.py checks them against the sources)
K_SF_STRIP, K_PK_BACK = 14, 64
K_SF_TILE = 64 * K_SF_STRIP
PK_SEG_RECS, PREP_RUN = 256, 8
K_DS_SUB, K_DS_J = 128, 8
K_DS_TILE = K_DS_SUB * K_DS_J
K_CHUNK_ROWS, DEC_TILE_ROWS = 64, 512

SEAMS = ("sift_tile", "sift_halo", "prep_run", "gain_seg", "dseg_sub", "dseg_tile", "dec64", "dec_tile")
SHAPES = ("R-bottom", "R-top", "R-plateau-first", "R-plateau-mid", "R-plateau-last", "R-swing", "R-gap", "R-first", "R-last", "R-skew")
KINDS = ("nrzi9", "nrzi7", "gcr", "pe", "ww")
SKEW = "3,1,2,0,3,0,1,2,1"
LADDER = (1.5, 2.2, 25.0, 100.0, 400.0)


def kernel_constants(root):
    """what the sources say the mirrored constants are: a dict of numbers and of the expressions they sit in"""
    src = lambda f: open(os.path.join(root, "readtape_amd", "csrc", f)).read()
    dev, api, dense = src("rtfe_device.h"), src("rtfe_api.hip"), src("rtfe_dense.hip")
    num = lambda s, name: int(re.search(r"\b" + name + r"\s*=\s*(\d+)\s*;", s).group(1))
    has = lambda s, text: text in s
    return dict(kSfStrip=num(dev, "kSfStrip"), kPkBack=num(dev, "kPkBack"), kChunkRows=num(dev, "kChunkRows"), kDsSub=num(dense, "kDsSub"), kDsJ=num(dense, "kDsJ"),
                sf_tile=has(dev, "kSfTile    = 64 * kSfStrip;"), ds_tile=has(dense, "kDsTile = kDsSub * kDsJ;"),
                hl=has(api, "d.pk_hl = (kPkBack + 2 * wmax + 6 + 7) & ~7;"), hr=has(api, "d.pk_hr = (wmax + 2 + 7) & ~7;"),
                seg_recs=num(api, r"d\.pk_seg_recs"), prep_run=has(api, 'h->prep_run = getenv("RTFE_PREP_RUN") ? atoi(getenv("RTFE_PREP_RUN")) : 8;'),
                dec_tile=has(api, "64 * (128 / (c->ntrks > 0 ? c->ntrks : 9)) : 512));"),
                window=has(api, "(int)(ps.pkww_bitfrac / (c->bpi * c->ips * d.sample_deltat));"))


def window(hdr, pset=0):
    """pkww_width of the built-in parameter set `pset` (src/readtape.c:1455-1457, as rtfe_api.hip computes it, in float)"""
    mode = {tbin.MODE_NRZI: frontend.NRZI, tbin.MODE_PE: frontend.PE, tbin.MODE_GCR: frontend.GCR}[hdr.mode]
    frac = np.float32(frontend.DEFAULT_PARMSETS[mode][pset][0])
    dt = np.float32(hdr.tdelta_ns) / np.float32(1e9)
    return min(50, int(frac / (np.float32(hdr.bpi) * np.float32(hdr.ips) * dt)))


def sift_halos(W):
    """(rows in front of, rows behind) a k_sift tile in LDS (rtfe_api.hip: pk_hl, pk_hr)"""
    return (K_PK_BACK + 2 * W + 6 + 7) & ~7, (W + 2 + 7) & ~7


def _edge(row, period):
    r = row % period
    return r <= 1 or r >= period - 2


def seams_of(row, W):
    """the seam classes row `row` lies on (all but gain_seg, which is counted in a track's peaks: shape_rows marks those sites itself)"""
    out = set()
    hl, hr = sift_halos(W)
    r = row % K_SF_TILE
    if _edge(row, K_SF_TILE):
        out.add("sift_tile")
    if r in (K_SF_TILE - hl, K_SF_TILE - hl + 1, hr - 2, hr - 1, K_SF_TILE - W, K_SF_TILE - W + 1, W, W + 1):      # (k_sift's halos; k_sift_s keeps W rows in front and W + 2 behind)
        out.add("sift_halo")
    if _edge(row, PREP_RUN * K_SF_TILE):
        out.add("prep_run")
    if _edge(row, K_DS_SUB):
        out.add("dseg_sub")
    if _edge(row, K_DS_TILE):
        out.add("dseg_tile")
    if _edge(row, K_CHUNK_ROWS):
        out.add("dec64")
    if _edge(row, DEC_TILE_ROWS):
        out.add("dec_tile")
    return out


def seam_rows(lo, hi, W):
    """every row of [lo, hi) that lies on a seam, with its classes"""
    return [(r, s) for r in range(lo, hi) for s in [seams_of(r, W)] if s]


def base_tape(kind, seed):
    """(hdr, rows, oracle options, [(first row, end row)] of the blocks) of a clean tape of about 20 000 rows; NRZI: one block long enough for a track's
    chain to run through several of k_gain_seg's segments"""
    if kind.startswith("nrzi"):
        n = 7 if kind == "nrzi7" else 9
        spec = synth.nrzi_spec(seed=seed, ntrks=n, noise_mv=0.0)
        rng = np.random.default_rng(seed + 1000)
        pay = synth.random_payloads(rng, 1, 690, 720, databits=n - 1) + synth.random_payloads(rng, 2, 30, 50, databits=n - 1)
        tape = synth.make_tape(spec, [("block", p) for p in pay], gap_samples=2000)
        opts = ["-ntrks=7"] if n == 7 else []
    elif kind == "gcr":
        tape = synth.gcr_tape(seed=seed, nblocks=2, minlen=60, maxlen=140, gap_samples=3000, noise_mv=0.0)
        opts = []
    elif kind == "pe":
        tape = synth.pe_tape(seed=seed, nblocks=3, minlen=60, maxlen=110, gap_samples=3000, noise_mv=0.0)
        opts = []
    elif kind == "ww":
        tape = synth.ww_tape(seed=seed, nblocks=6, minwords=3, maxwords=10, marks_every=3, gap_samples=700, noise_mv=0.0)
        opts = []
    else:
        raise ValueError(kind)
    return tape.spec.header(), np.ascontiguousarray(tape.rows), opts, [(int(b[1]), int(b[2])) for b in tape.blocks]


def to_int16(x):
    """clipped to the int16 range; column 0 stops at -32767 (-32768 there is the TBIN end mark)"""
    x = np.clip(x, -32768, 32767)
    x[:, 0] = np.maximum(x[:, 0], -32767)
    return np.ascontiguousarray(x.astype(np.int16))


def clipped(rows, k):
    """rows x k, clipped: every excursion beyond 1 / k of full scale a plateau on a rail"""
    return to_int16(rows.astype(np.int64) * k)


def rescaled(hdr, rows, maxvolts):
    """the same voltages digitised at `maxvolts` full scale (rounded, clipped at the rails)"""
    return dataclasses.replace(hdr, maxvolts=maxvolts), to_int16(np.rint(rows.astype(np.float64) * (hdr.maxvolts / maxvolts)).astype(np.int64))


def without_rail(rows):
    """the tape as a digitiser that stops at -32767 would have delivered it"""
    return np.ascontiguousarray(np.maximum(rows, -32767))


def _extremes(x, sign, floor):
    s = sign * x.astype(np.int64)
    return np.flatnonzero((s[1:-1] > s[:-2]) & (s[1:-1] >= s[2:]) & (s[1:-1] > floor)) + 1


def shape_rows(hdr, rows0, blocks, rng, skew=None, density=0.03):
    """rows0 with single rail samples and short rail plateaus at the seams of every second block (the first, the third ...: the bursts of the others stay
    free of -32768) and at a share (`density`) of its other extremes.  Returns (rows, sites); a site = dict(row, trk (head), shape, seams)."""
    rows = rows0.astype(np.int64).copy()
    nrows, ntrks = rows.shape
    W = window(hdr) if hdr.mode != tbin.MODE_WW else 8
    sites = []
    busy = np.zeros((nrows, ntrks), bool)
    all_blocks, blocks = blocks, blocks[::2]
    bots = {t: _extremes(rows0[:, t], -1, 0.4 * np.abs(rows0[:, t]).max()) for t in range(1, ntrks)}
    tops = {t: _extremes(rows0[:, t], 1, 0.4 * np.abs(rows0[:, t]).max()) for t in range(1, ntrks)}

    def site(r, t, shape, seams=()):
        sites.append(dict(row=int(r), trk=int(t), shape=shape, seams=tuple(sorted(seams))))

    def plateau(r, t, P):
        """the bottom at row P of head t stretched to row r, where its one -32768 sits"""
        a, b = min(P, r), max(P, r)
        if busy[max(a - 3, 0):b + 4, t].any():
            return False
        mid = P != r and abs(P - r) <= 2 and rng.random() < 0.5
        if mid:
            a, b = r - 2, r + 2
        rows[a:b + 1, t] = -32767
        rows[r, t] = -32768
        busy[max(a - 3, 0):b + 4, t] = True
        site(r, t, "R-bottom" if a == b else ("R-plateau-mid" if mid else ("R-plateau-first" if r == a else "R-plateau-last")), seams_of(r, W))
        return True

    # the seams inside the blocks: the head >= 1 whose bottom lies nearest takes the site
    for lo, hi in blocks:
        for r, cls in seam_rows(lo + 2 * W, hi - 2 * W, W):
            if rng.random() < 0.85 and not ({"sift_tile", "sift_halo", "prep_run", "dseg_tile", "dec_tile"} & cls):      # (the 64- and 128-row grids are dense: a share of their rows will do)
                continue
            cand = []
            for t in range(1, ntrks):
                b = bots[t]
                if b.size:
                    k = int(np.argmin(np.abs(b - r)))
                    cand.append((abs(int(b[k]) - r), t, int(b[k])))
            cand.sort()
            for d, t, P in cand[:3]:
                if d <= 8 and plateau(r, t, P):
                    break
    # k_gain_seg: a chain's steady stretch is cut every PK_SEG_RECS records, counted from where its baseline was fixed (some twenty peaks into
    # the block): every bottom of a stretch of peaks around each multiple is a site, whichever record the count started at
    for lo, hi in blocks:
        for t in range(1, ntrks):
            pk = np.sort(np.concatenate([bots[t], tops[t]]))
            pk = pk[(pk >= lo) & (pk < hi)]
            for j in range(1, pk.size // PK_SEG_RECS + 1):
                for P in pk[j * PK_SEG_RECS - 6:j * PK_SEG_RECS + 30]:
                    if rows0[P, t] < 0 and not busy[P - 3:P + 4, t].any():
                        rows[P, t] = -32768
                        busy[P - 3:P + 4, t] = True
                        site(P, t, "R-bottom", seams_of(int(P), W) | {"gain_seg"})
    # random extremes inside the blocks: single bottoms and tops, full-scale swings
    for t in range(1, ntrks):
        for P in bots[t]:
            if rng.random() < density and not busy[P - 3:P + 5, t].any() and any(lo < P < hi - 2 for lo, hi in blocks):
                if rng.random() < 0.4:
                    rows[P, t] = -32768; rows[P + 1, t] = 32767
                    site(P, t, "R-swing", seams_of(int(P), W))
                else:
                    rows[P, t] = -32768
                    site(P, t, "R-bottom", seams_of(int(P), W))
                busy[P - 3:P + 5, t] = True
        for P in tops[t]:
            if rng.random() < density and not busy[P - 3:P + 4, t].any() and any(lo < P < hi for lo, hi in blocks):
                rows[P, t] = 32767
                busy[P - 3:P + 4, t] = True
                site(P, t, "R-top")
    # a lone -32768 in the middle of the gap behind every shaped block; the tape's first and last row
    ends = [0] + [hi for _, hi in all_blocks]
    starts = [lo for lo, _ in all_blocks] + [nrows]
    for i, (a, b) in enumerate(zip(ends, starts)):
        if i % 2 == 1 and i < len(all_blocks) and b - a > 600:
            t = int(rng.integers(1, ntrks))
            r = (a + b) // 2 + int(rng.integers(-40, 41))
            rows[r, t] = -32768
            site(r, t, "R-gap", seams_of(r, W))
    t = int(rng.integers(1, ntrks))
    rows[0, t] = -32768
    site(0, t, "R-first")
    t = int(rng.integers(1, ntrks))
    rows[nrows - 1, t] = -32768
    site(nrows - 1, t, "R-last")
    if skew:                                                    # inside the deskew delay: the FIFO hands the tape's first rows through undelayed
        for t in range(1, ntrks):
            if skew[t] >= 2:
                rows[skew[t] - 1, t] = -32768
                site(skew[t] - 1, t, "R-skew")
    return to_int16(rows), sites


def coverage(rows, sites, W):
    """{class: count}: the shape classes of the sites as written, the seam classes of every -32768 sample of the tape (a plateau's too)"""
    cnt = {}
    for s in sites:
        cnt[s["shape"]] = cnt.get(s["shape"], 0) + 1
        if "gain_seg" in s["seams"]:
            cnt["gain_seg"] = cnt.get("gain_seg", 0) + 1
    for r in np.flatnonzero((rows == -32768).any(1)):
        for sm in seams_of(int(r), W):
            cnt[sm] = cnt.get(sm, 0) + 1
    return cnt


def draw(seed):
    """the parameters of tape `seed` (one place: the tool and the tests draw the same tapes)"""
    rng = np.random.default_rng(seed + 9_000_000)
    kind = str(rng.choice(KINDS))
    d = dict(kind=kind, how=str(rng.choice(["x2", "x4", "sparse", "sparse"])), invert=bool(rng.random() < 0.7))
    d["skew"] = kind == "nrzi9" and rng.random() < 0.3
    d["m"] = kind == "nrzi9" and not d["skew"] and rng.random() < 0.25
    d["fluxdir"] = str(rng.choice(["neg", "pos", "auto"])) if kind == "ww" else None
    return d


def shaped(seed, **over):
    """(hdr, rows, sites, oracle options, blocks) of tape `seed`"""
    d = draw(seed)
    d.update(over)
    hdr, rows0, opts, blocks = base_tape(d["kind"], seed)
    skew = [int(x) for x in SKEW.split(",")] if d["skew"] else None
    if d["how"] == "sparse":
        rows, sites = shape_rows(hdr, rows0, blocks, np.random.default_rng(seed * 7919 + 29), skew=skew)
    else:
        rows, sites = clipped(rows0, int(d["how"][1:]) + (d["kind"] == "ww")), []      # (Whirlwind pulses are 2 V of 4.4: x3 and x4 clip them)
    opts = opts + (["-invert"] if d["invert"] else []) + ([f"-skew={SKEW}"] if skew else []) + (["-m"] if d["m"] else [])
    if d["fluxdir"]:
        opts.append(f"-fluxdir={d['fluxdir']}")
    return hdr, rows, sites, opts, blocks


def rail_bursts(rows, bursts):
    """per burst of a scan: do the rows it walked, [reset_sample, end_sample), hold a -32768?"""
    has = (rows == -32768).any(1)
    return np.array([bool(has[int(b["reset_sample"]):int(b["end_sample"])].any()) for b in bursts], bool)


def run_oracle(hdr, rows, opts, wd):
    """the oracle's run of the tape: (exit code, its transitions, its .tap bytes)"""
    import subprocess
    import refdump
    from parity_util import ORACLE, build_oracle
    build_oracle()
    os.makedirs(wd, exist_ok=True)
    tbin.write_tbin(os.path.join(wd, "t.tbin"), hdr, rows)
    p = subprocess.run([ORACLE, "-v", f"-out={wd}/o", f"-evt={wd}/o.evt"] + list(opts) + [os.path.join(wd, "t.tbin")], capture_output=True, text=True)
    assert p.returncode in (0, 99), p.stderr
    tap = open(os.path.join(wd, "o.tap"), "rb").read() if os.path.exists(os.path.join(wd, "o.tap")) else b""
    return p.returncode, refdump.load(os.path.join(wd, "o.evt")), tap


def e2e(hdr, rows, opts, wd, fe_factory=None, chunk_rows=4096):
    """The whole pipeline - front end, replay, block decoders, .tap writer - against the oracle: the transitions the decoders were handed and the .tap
    bytes.  Returns (mismatches, the oracle's transitions)."""
    import refdump
    from readtape_amd import pipeline
    rc, b, otap = run_oracle(hdr, rows, opts, wd)
    invert = "-invert" in opts
    try:
        if hdr.mode == tbin.MODE_WW:
            pipeline.decode_tape_ww(hdr, rows, os.path.join(wd, "g.tap"), evt_path=os.path.join(wd, "g.evt"), fe_factory=fe_factory, invert=invert, chunk_rows=chunk_rows,
                                    fluxdir=next((a[9:] for a in opts if a.startswith("-fluxdir=")), "neg"))
        else:
            pipeline.decode_tape(hdr, rows, os.path.join(wd, "g.tap"), evt_path=os.path.join(wd, "g.evt"), fe_factory=fe_factory, invert=invert,
                                 opts=pipeline.DecodeOptions(multiple_tries="-m" in opts),
                                 skew=next(([int(x) for x in a[6:].split(",")] for a in opts if a.startswith("-skew=")), None))
    except pipeline.ReferenceFatal:                            # what is fatal in the reference (exit 99) must be fatal here too
        if rc != 99:
            return ["the pipeline stopped at a reference assert, the oracle did not"], b
    a = refdump.load(os.path.join(wd, "g.evt"))
    msgs = []
    if rc == 0:
        if open(os.path.join(wd, "g.tap"), "rb").read() != otap:
            msgs.append(".tap differs")
    else:
        n = min(a.size, b.size)
        a, b = a[:n], b[:n]
    return msgs + refdump.compare(a, b), b
