"""Shapes written over the sign changes of tapes decoded with -zeros and -zeros -differentiate: the inputs of tools/fuzz_shapes.py --zeros / --diffz and of
tests/test_*_zeros_shapes.py.  Test infrastructure.

The zero-crossing detectors (src/decoder.c:617-649 and 654-683) run speculatively in parallel on the device: k_zeros (rtfe_zeros.hip) cuts a burst into a
sequential head of KZP_HEAD rows, sub-segments of KZP_SUB rows that start zc_warm rows early from a fresh state, and a tail; k_decode's zero-crossing mode
(rtfe_kernels.hip: -invert, deskew, one track) cuts tiles of zc_tile_rows() rows into sub-segments of KZC_SUB rows.  Gaussian noise rarely lands the shapes
that decide a crossing - exact zeros, extremes one code either side of the threshold, a top that returns to the same value, a crossing that stays armed for
longer than a sub-segment - on those seams.  shape_rows() writes them there and at random sign changes; every site records its row, track, shape class and
seam class, so that a test can assert what its tapes covered."""
import dataclasses
import os
import re

import numpy as np

from readtape_amd import synth

# the seams, mirrored from the kernels (test_emul_zeros_shapes.py checks them against the sources)
KZP_HEAD, KZP_SUB, KZC_SUB = 32, 128, 64
K_MARGIN_ROWS, K_MAX_TILE_ROWS = 256, 2048

SHAPES = ("Z-zero", "Z-edge", "Z-equal", "Z-flicker", "Z-slow", "Z-sub", "Z-slope", "Z-rail")
DIFF_SHAPES = ("D-run", "D-band", "D-skip")
SEAMS = ("zp_head", "zp_sub", "zp_warm", "zp_tail", "zc_sub", "zc_tile", "odd_col", "unaligned_pair")
KINDS = ("pe", "nrzi9", "nrzi7", "gcr")
MAXVOLTS = (2.5, 3.3, 4.4, 10.0, 0.37)


def zc_tile_rows(ntrks):
    """k_decode's tile rows for -zeros without -differentiate (rtfe_api.hip: 64 * (128 / ntrks), on the 64-row grid, kMarginRows .. kMaxTileRows)"""
    tr = (64 * (128 // ntrks)) // 64 * 64
    return min(max(tr, K_MARGIN_ROWS), K_MAX_TILE_ROWS)


def zc_warm(hdr):
    """rows a k_zeros sub-segment starts early (rtfe_api.hip: two bit cells, a multiple of 8, 16 .. 64)"""
    spbw = np.float32(1.0) / (np.float32(hdr.bpi) * np.float32(hdr.ips) * np.float32(hdr.tdelta_ns * 1e-9))
    w = (int(np.float32(2.0) * spbw) + 7) & ~7
    return min(max(w, 16), 64)


def volt(code, maxvolts):
    """the reference's conversion (src/readtape.c:1420): (float)c / 32767 * maxvolts, in float"""
    return np.float32(code) / np.float32(32767) * np.float32(maxvolts)


def zc_peak_code(maxvolts):
    """the smallest c in 1 .. 32768 with volt(c) > ZEROCROSS_PEAK (0.2 V): a top confirms at c >= P, a bottom at c <= -P; 32769: no code does"""
    c = np.arange(1, 32769, dtype=np.int64)
    ok = np.flatnonzero(volt(c, maxvolts) > np.float32(0.2))
    return int(c[ok[0]]) if ok.size else 32769


def kernel_constants(root):
    """(kZpHead, kZpSub, kZcSub, the -zeros tile-row expression) as the sources have them"""
    src = lambda f: open(os.path.join(root, "readtape_amd", "csrc", f)).read()
    z, k, a = src("rtfe_zeros.hip"), src("rtfe_kernels.hip"), src("rtfe_api.hip")
    num = lambda s, name: int(re.search(r"\b" + name + r"\s*=\s*(\d+)", s).group(1))
    tile = re.search(r"\(c->find_zeros && !c->differentiate\) \? (64 \* \(128 / \(c->ntrks > 0 \? c->ntrks : 9\)\)) : 512", a)
    tile = tile.group(1) if tile else None
    return num(z, "kZpHead"), num(z, "kZpSub"), num(k, "kZcSub"), tile


def burst_spans(bursts, nrows, tail_rows):
    """[(restart, stop)] of k_zeros' bursts: it walks from the restart to the next burst's restart, at most tail_rows into the next quiet zone"""
    out = []
    for i, b in enumerate(bursts):
        stop = nrows
        if i + 1 < len(bursts):
            nb = bursts[i + 1]
            stop = min(int(nb["zone_end"]) - K_MARGIN_ROWS, int(nb["zone_first"]) + tail_rows)
        out.append((int(b["reset_sample"]), min(stop, nrows)))
    return out


def seams_of(row, col, ntrks, spans, warm):
    """the seam classes row `row` of column `col` lies on, given burst_spans() of a scan"""
    out = set()
    for reset, end in spans:
        if not (reset <= row < end):
            continue
        c0 = reset + KZP_HEAD
        if abs(row - c0) <= 2:
            out.add("zp_head")
        k = row - c0
        if k > 0:
            j, r = divmod(k, KZP_SUB)
            if j >= 1 and (r <= 2 or r >= KZP_SUB - 2) or (j == 0 and r >= KZP_SUB - 2):
                out.add("zp_sub")
            if r >= KZP_SUB - warm:
                out.add("zp_warm")
        if k >= 0 and row >= c0 + (end - c0) // KZP_SUB * KZP_SUB:
            out.add("zp_tail")
    if any(a <= row < b for a, b in spans):
        if row % KZC_SUB <= 2 or row % KZC_SUB >= KZC_SUB - 2:
            out.add("zc_sub")
        t = zc_tile_rows(ntrks)
        if row % t <= 2 or row % t >= t - 2:
            out.add("zc_tile")
    if ntrks & 1 and col == ntrks - 1:
        out.add("odd_col")
    col0 = ntrks - 2 if (ntrks & 1 and col == ntrks - 1) else col & ~1
    if (2 * ntrks * row + 2 * col0) % 4:
        out.add("unaligned_pair")
    return out


def tail_rows(hdr):
    """rows of the next quiet zone a burst's walk still takes (rtfe_api.hip: 48 bit cells)"""
    return 48 * max(1, int(1 / (np.float32(hdr.bpi) * np.float32(hdr.ips) * np.float32(hdr.tdelta_ns * 1e-9))))


def coverage(sites, hdr, nrows, bursts):
    """{class: count} over the sites: shape classes as written, seam classes recomputed against `bursts`"""
    cnt = {}
    spans = burst_spans(bursts, nrows, tail_rows(hdr))
    for s in sites:
        cnt[s["shape"]] = cnt.get(s["shape"], 0) + 1
        for sm in seams_of(s["row"], s["trk"], hdr.ntrks, spans, zc_warm(hdr)):
            cnt[sm] = cnt.get(sm, 0) + 1
    return cnt


def base_tape(kind, seed, noise_mv, maxvolts, ntrks=None):
    """(hdr, rows, oracle options) of a short tape; the samples rescaled to `maxvolts` full scale (clipped at the rails).  ntrks: the columns of a PE
    tape repeated or cut to that many (path against path only: the oracle decodes 7 and 9 tracks)"""
    if kind.startswith("nrzi"):
        n = 7 if kind == "nrzi7" else 9
        tape = synth.nrzi_tape(seed=seed, nblocks=2, minlen=60, maxlen=160, gap_samples=2500, noise_mv=noise_mv, ntrks=n)
    elif kind == "gcr":
        tape = synth.gcr_tape(seed=seed, nblocks=2, minlen=40, maxlen=120, gap_samples=3000, noise_mv=noise_mv)
    else:
        tape = synth.pe_tape(seed=seed, nblocks=2, minlen=40, maxlen=120, gap_samples=3000, noise_mv=noise_mv)
    hdr = tape.spec.header()
    rows = np.clip(np.rint(tape.rows.astype(np.float64) * (hdr.maxvolts / maxvolts)), -32767, 32767).astype(np.int16)
    hdr = dataclasses.replace(hdr, maxvolts=maxvolts)
    opts = ["-ntrks=7"] if kind == "nrzi7" else []
    if ntrks is not None and ntrks != rows.shape[1]:
        rows = np.ascontiguousarray(np.concatenate([rows] * (ntrks // rows.shape[1] + 1), 1)[:, :ntrks])
        hdr = dataclasses.replace(hdr, ntrks=ntrks)
    return hdr, np.ascontiguousarray(rows), opts


def _sign_changes(x, lo=64):
    s = np.sign(x.astype(np.int64))
    at = np.flatnonzero((s[1:] * s[:-1] < 0)) + 1
    return at[at >= lo]


def shape_rows(hdr, rows0, bursts, rng, diff=False, density=0.04, per_seam=2):
    """rows0 with shapes over a share (`density`) of its in-block sign changes and at every burst's seams (`per_seam` sites a seam position);
    bursts = the burst table of a -zeros scan of rows0.  Returns (rows, sites)."""
    rows = rows0.astype(np.int64).copy()
    nrows, ntrks = rows.shape
    mv = hdr.maxvolts
    P = zc_peak_code(mv)
    Pc = min(P, 32767)
    spb = max(4, int(1.0 / (hdr.bpi * hdr.ips * hdr.tdelta_ns * 1e-9)))
    warm = zc_warm(hdr)
    band = max(1, int(round(0.05 * 32767 / mv)))             # the differentiator's dead band in codes (src/readtape.c:1386)
    classes = DIFF_SHAPES + ("Z-zero", "Z-flicker", "Z-rail") if diff else SHAPES
    sites = []
    busy = np.zeros((nrows, ntrks), bool)

    def amp(t):
        return int(min(32767, max(Pc + 64, 0.8 * np.abs(rows0[:, t]).max())))

    def put(r, t, v):
        if 0 <= r < nrows:
            if t == 0 and v < -32767:
                v = -32767                                     # (column 0 at -32768 is the TBIN end mark)
            rows[r, t] = int(np.clip(v, -32768, 32767))

    def write(cls, r, t, sg, quiet=False):
        """shape `cls` with the sign change (-sg -> +sg) at row r of column t; returns the rows it spans.  quiet: inside a quiet zone (a burst's
        head, its tail): exact zeros and +-1 flickers only, which leave the zone - and so the burst table - as it was"""
        if quiet:
            m = int(rng.integers(2, 7))
            for k in range(m):
                put(r + k, t, 0 if cls == "Z-zero" else (sg if k % 2 == 0 else -sg))
            return r, r + m
        A = amp(t)
        lead = max(3, spb // 2)
        for k in range(1, lead + 1):                             # the excursion in front: an extreme beyond the threshold arms the crossing
            put(r - k, t, -sg * (A if k == lead // 2 + 1 else max(1, A * k // (lead + 1))))
        if cls == "Z-zero":
            v = int(rng.integers(0, 3))
            if v == 0:
                for k in range(int(rng.integers(1, 5))):
                    put(r + k, t, 0)
                r2 = r + 4
            elif v == 1:
                put(r, t, sg); put(r + 1, t, 0); r2 = r + 2          # a zero right behind the arming row
            else:
                put(r - 1, t, 0); r2 = r                              # a zero as v_prev
            for k in range(spb // 2):
                put(r2 + k, t, sg * max(1, A * (k + 1) // (spb // 2)))
            return r - lead, r2 + spb // 2
        if cls == "Z-edge":
            d = int(rng.integers(-2, 3))
            pk = sg * (P + d)
            if rng.random() < 0.5:
                put(r - lead // 2 - 1, t, -pk)                       # the arming extreme at the edge
            for k in range(spb // 2):
                put(r + k, t, pk if k == spb // 4 else sg * max(1, abs(pk) * (k + 1) // (spb // 2 + 2)))
            return r - lead, r + spb // 2
        if cls == "Z-equal":
            v = sg * (Pc + int(rng.integers(0, 3)))
            n = int(rng.integers(2, 7))
            put(r, t, sg * max(1, Pc // 2))
            for k in range(1, n + 1):
                put(r + k, t, v if k % 2 else sg * (Pc // 2 + k))           # the top back to the same value, dips between
            end = r + n + 1
            if rng.random() < 0.6:
                put(end, t, v + sg); end += 1                         # ... and then a new extreme
            return r - lead, end
        if cls == "Z-flicker":
            m = int(rng.integers(2, 8))
            for k in range(m):
                put(r + k, t, sg if k % 2 == 0 else -sg)
            for k in range(spb // 2):
                put(r + m + k, t, sg * max(1, A * (k + 1) // (spb // 2)))
            return r - lead, r + m + spb // 2
        if cls in ("Z-slow", "Z-sub"):
            L = int(rng.integers(KZP_SUB + warm + 8, 2 * KZP_SUB + warm)) if cls == "Z-slow" else int(rng.integers(KZP_SUB // 2, 2 * KZP_SUB))
            v = sg * (max(1, Pc // 3) if cls == "Z-slow" else max(1, Pc - 1))
            for k in range(L):
                put(r + k, t, v)
            put(r + L, t, sg * A)
            return r - lead, r + L + 1
        if cls == "Z-slope":
            D = int(round(1.5 * spb)) + int(rng.integers(-3, 4))
            for k in range(D):
                put(r + k, t, sg * max(1, Pc // 3))
            put(r + D, t, sg * A)
            return r - lead, r + D + 1
        if cls == "Z-rail":
            if sg > 0:
                put(r - lead // 2 - 1, t, -32768); put(r + 1, t, 32767)
            else:
                put(r - lead // 2 - 1, t, 32767); put(r + 1, t, -32768)
            put(r, t, sg * max(1, A // 3))
            return r - lead, r + 2
        if cls == "D-run":
            k = int(rng.integers(1, 7))
            up = max(2, spb // 3)
            for i in range(up):
                put(r + i, t, sg * A * (i + 1) // up)
            for i in range(k):
                put(r + up + i, t, sg * A)                            # flat raw samples: exact zeros after the differentiator
            for i in range(up):
                put(r + up + k + i, t, sg * A - 2 * sg * A * (i + 1) // up)
            return r - lead, r + 2 * up + k
        if cls == "D-band":
            e = int(rng.integers(-1, 2))
            v = int(rows[r - 1, t]) if r > 0 else 0
            n = int(rng.integers(3, 9))
            for i in range(n):
                v += sg * (band + e) * (1 if i % 3 else 2)
                put(r + i, t, v)
            return r - lead, r + n
        raise ValueError(cls)

    def place(cls, r, t, seam, quiet=False):
        if r < spb + 8 or r + 8 >= nrows or (not quiet and r + 3 * KZP_SUB >= nrows):
            return
        lo, hi = r - spb - 4, r + (2 * KZP_SUB + warm + 8 if cls in ("Z-slow", "Z-sub") else 2 * spb + 12)
        if busy[max(lo, 0):min(hi, nrows), t].any():
            return
        sg = 1 if rng.random() < 0.5 else -1
        a, b = write(cls, r, t, sg, quiet)
        busy[max(a - 2, 0):min(b + 2, nrows), t] = True
        sites.append(dict(row=int(r), trk=int(t), shape=cls, seam=seam, sign=sg))

    spans = burst_spans(bursts, nrows, tail_rows(hdr))
    live = [(int(b["zone_end"]), int(bursts[i + 1]["zone_first"]) if i + 1 < len(bursts) else nrows) for i, b in enumerate(bursts)]
    blocks = [(a, min(b, e)) for (a, b), (_, e) in zip(live, spans)]
    # seams first: where they lie in a quiet zone (the head, the tail) only quiet shapes, which leave the burst table alone
    for (reset, stop), (lo, hi) in zip(spans, live):
        c0 = reset + KZP_HEAD
        targets = [("zp_head", c0 + int(rng.integers(-2, 3)))]
        for j in range(1, (stop - c0) // KZP_SUB + 1):
            s0 = c0 + j * KZP_SUB
            targets.append(("zp_sub", s0 + int(rng.integers(-2, 3))))
            targets.append(("zp_warm", s0 - int(rng.integers(1, warm + 1))))
        tail0 = c0 + (stop - c0) // KZP_SUB * KZP_SUB
        if stop - tail0 > 8:
            targets.append(("zp_tail", int(rng.integers(tail0, stop - 7))))
        g = (lo // KZC_SUB + 1) * KZC_SUB
        while g < hi:
            targets.append(("zc_tile" if g % zc_tile_rows(ntrks) == 0 else "zc_sub", g + int(rng.integers(-2, 3))))
            g += KZC_SUB * int(rng.integers(1, 3))
        g = (lo // zc_tile_rows(ntrks) + 1) * zc_tile_rows(ntrks)
        while g < hi:
            targets.append(("zc_tile", g + int(rng.integers(-2, 3))))
            g += zc_tile_rows(ntrks)
        for seam, r in targets:
            quiet = not (lo + spb < r < hi - 2 * spb)
            if quiet and not (reset <= r < stop):
                continue
            for _ in range(per_seam):
                t = ntrks - 1 if (ntrks & 1 and rng.random() < 0.3) else int(rng.integers(0, ntrks))
                cls = str(rng.choice(["Z-zero", "Z-flicker"] if quiet else [c for c in classes if c != "D-skip"]))
                place(cls, r, t, seam, quiet)
        end = hi
        if diff:                                                 # the interblock skip right behind the block's end (Q11)
            for _ in range(per_seam):
                t = int(rng.integers(0, ntrks))
                r = end + int(rng.integers(2, 40))
                if r + 8 < nrows and not busy[r - 4:r + 8, t].any():
                    A = amp(t)
                    for k, v in enumerate((A // 2, A, A // 2, 0, -A // 2, -A, -A // 2)):
                        put(r + k, t, v)
                    busy[r - 4:r + 8, t] = True
                    sites.append(dict(row=int(r), trk=int(t), shape="D-skip", seam="skip", sign=1))
    # random sign changes inside the blocks
    for t in range(ntrks):
        for r in _sign_changes(rows0[:, t]):
            if rng.random() < density and any(a + spb < r < b - spb for a, b in blocks):
                place(str(rng.choice([c for c in classes if c != "D-skip"])), int(r), t, "random")
    # runs of exact zeros on the tape's first rows (tstart 0: the t_firstzero == 0 sentinel of src/decoder.c:658)
    if diff and rng.random() < 0.5:
        t = int(rng.integers(0, ntrks))
        A = amp(t)
        for k in range(12):
            rows[k, t] = 0
        for k in range(12, 20):
            rows[k, t] = A if k < 16 else -A
        sites.append(dict(row=0, trk=t, shape="D-run", seam="tape_start", sign=1))
    return rows.astype(np.int16), sites


def draw(seed):
    """the parameters of tape `seed` (one place: the tool and the tests draw the same tapes)"""
    rng = np.random.default_rng(seed + 5_000_000)
    return dict(kind=str(rng.choice(KINDS)), noise_mv=float(rng.choice([0.0, 5.0, 30.0])), maxvolts=float(rng.choice(MAXVOLTS)),
                density=float(rng.choice([0.02, 0.05, 0.1])))


def shaped(seed, scan, diff=False, ntrks=None, **over):
    """(hdr, rows0, rows, sites, oracle options) of tape `seed`; scan(hdr, rows) -> the burst table of a -zeros scan (the placement's yardstick)"""
    d = draw(seed)
    d.update(over)
    hdr, rows0, opts = base_tape(d["kind"], seed, d["noise_mv"], d["maxvolts"], ntrks=ntrks)
    rows, sites = shape_rows(hdr, rows0, scan(hdr, rows0), np.random.default_rng(seed * 7919 + 17), diff=diff, density=d["density"])
    return hdr, rows0, rows, sites, opts + ["-zeros"] + (["-differentiate"] if diff else [])


def e2e(hdr, rows, opts, wd, fe_factory=None):
    """The whole pipeline against the oracle, as tests/stress_gpu.py compares -zeros: the transitions the decoders were handed (-evt) and the .tap bytes.
    Returns (mismatches, the oracle's transitions)."""
    import subprocess
    import refdump
    from parity_util import ORACLE, build_oracle
    from readtape_amd import pipeline, tbin
    build_oracle()
    os.makedirs(wd, exist_ok=True)
    tbin.write_tbin(os.path.join(wd, "t.tbin"), hdr, rows)
    p = subprocess.run([ORACLE, "-v", f"-out={wd}/o", f"-evt={wd}/o.evt"] + opts + [os.path.join(wd, "t.tbin")], capture_output=True, text=True)
    b = refdump.load(os.path.join(wd, "o.evt"))
    try:
        pipeline.decode_tape(hdr, rows, os.path.join(wd, "g.tap"), evt_path=os.path.join(wd, "g.evt"), find_zeros=True, differentiate="-differentiate" in opts,
                             invert="-invert" in opts, skew=next(([int(x) for x in a[6:].split(",")] for a in opts if a.startswith("-skew=")), None), fe_factory=fe_factory)
    except RuntimeError as e:                                  # what is fatal in the reference (exit 99) must be fatal here too
        ok = p.returncode == 99 and ("no transitions" in str(e) or "non-standard" in str(e) or "non-positive" in str(e))
        return ([] if ok else [f"pipeline raised {e!r}, oracle rc {p.returncode}"]), b
    a = refdump.load(os.path.join(wd, "g.evt"))
    msgs = []
    if p.returncode == 0:
        if open(os.path.join(wd, "g.tap"), "rb").read() != open(os.path.join(wd, "o.tap"), "rb").read():
            msgs.append(".tap differs")
    else:
        msgs += [] if p.returncode == 99 else [f"oracle rc {p.returncode}"]
        n = min(a.size, b.size)
        a, b = a[:n], b[:n]
    ign = ("v_avg_height",) if "-differentiate" in opts else ()
    return msgs + refdump.compare(a, b, ignore_fields=ign), b
