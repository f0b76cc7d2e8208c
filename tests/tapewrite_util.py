"""What the host, the emulated and the GPU tests of the tape writer (readtape_amd/tapewrite.py; csrc/host/rt_tapewrite.c; the kernel in csrc/rtfe_tapewrite.hip)
share: the tapes that are written and decoded again, and the cases the device renderer is held against the host renderer on, byte for byte - every mode, raw
masks at six track counts, windows that leave partial 16-byte vectors at both ends, blocks and pulses at the seams of the kernel's spans, the rails, gaps
only, guard bytes, refusals."""
import ctypes as C
import os

import numpy as np

from readtape_amd import frontend, tapewrite as W, tbin, textfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "readtape_ref")
SKEW = tuple(0.1 * ((t * 3) % 5 - 2) for t in range(19))                 # -0.2 .. 0.2 cells, no two neighbours alike


def payload(seed, n, bits=8, lo=0):
    return bytes(np.random.default_rng(seed).integers(lo, 1 << bits, size=n, dtype=np.int64).astype(np.uint8))


# ---- the tapes that go through the decoders (test_tapewrite_host.py: the reference; test_gpu_tapewrite.py: this package's) ----
# A tape mark first, last and doubled; records of odd and even length from a dozen bytes to more than 4096; noise 10 mV and jitter 0.02 cells (the
# specs' defaults).  The shortest NRZI record is 3 bytes: with its 8 trailer cells a shorter one is a block of 10 cells or fewer, which the reference (and
# rt_decode_nrzi.c) drops as noise - the encoder refuses it (test_tapewrite_host.py::test_what_the_formats_cannot_carry).  PE and GCR take a record of one byte.
def tape_items(bits, lens, seed):
    recs = [("block", payload(seed + i, n, bits, lo=1 if bits < 8 else 0)) for i, n in enumerate(lens)]
    return [("mark",), recs[0], recs[1], ("mark",), ("mark",)] + recs[2:] + [("mark",)]


TAPES = {
    "nrzi9": (lambda: W.nrzi_spec(seed=11, gap_samples=3000), tape_items(8, (12, 13, 4097, 3, 300), 100), ()),
    "nrzi7": (lambda: W.nrzi_spec(seed=12, ntrks=7, gap_samples=3000), tape_items(6, (12, 13, 4097, 3, 300), 200), ()),
    "nrzi9_even": (lambda: W.nrzi_spec(seed=13, gap_samples=3000, even=True), tape_items(7, (12, 13, 4096, 5), 300), ("-even",)),
    "pe": (lambda: W.pe_spec(seed=14, gap_samples=3000), tape_items(8, (12, 13, 4097, 1, 300), 400), ()),
    "gcr": (lambda: W.gcr_spec(seed=15, gap_samples=3000), tape_items(8, (12, 13, 4097, 1, 2, 7, 300), 500), ()),
}


def same_items(want_img, got_img):
    """-> None, or what differs: the records (with their bytes and error flags) and tape marks of two .tap images, as textfile.read_tap gives them"""
    want, got = textfile.read_tap(want_img), textfile.read_tap(got_img)
    a = [(int(i["kind"]), int(i["flag"]), bytes(want_img[int(i["offset"]): int(i["offset"]) + int(i["length"])])) for i in want]
    b = [(int(i["kind"]), int(i["flag"]), bytes(got_img[int(i["offset"]): int(i["offset"]) + int(i["length"])])) for i in got]
    if a == b:
        return None
    return f"{len(b)} items for {len(a)}: " + ", ".join(f"{k}/{f}/{len(d)}" for k, f, d in b[:20]) + " for " + ", ".join(f"{k}/{f}/{len(d)}" for k, f, d in a[:20])


# ---- the device renderer's cases ----
class Device:
    """rtfe_tape_render of one library through one backend (the GPU's, or the emulator's), results as numpy."""

    def __init__(self, be, lib_path=None):
        self.be, self.lib_path = be, lib_path
        self.lib = W._bind(frontend._load_library(lib_path))
        self.torch = getattr(be, "torch", None)

    def span(self, ntrks):
        return int(self.lib.rtfe_tape_render_span_rows(ntrks))

    def host(self, t):
        return t.cpu().numpy() if self.torch is not None else np.asarray(t)

    def render(self, plan, first_row=0, nrows=None):
        return self.host(W.render_device(plan, first_row, nrows, _lib_path=self.lib_path, _backend=self.be))

    def buffer(self, nbytes, fill=0x5A):
        """nbytes of device memory from a 16-byte boundary with 64 guard bytes either side, all of them `fill` -> (the whole view, the offset of the payload)"""
        buf = self.be.empty(nbytes + 160)
        off = 64 + (-(self.be.ptr(buf) + 64) % 16)
        if self.torch is not None:
            buf.fill_(fill)
        else:
            buf[...] = fill
        return buf, off

    def guarded(self, plan, first_row, nrows):
        """the window rendered between guard bytes -> (rows, True if every guard byte is intact)"""
        nb = nrows * plan.params.ntrks * 2
        buf, off = self.buffer(nb)
        rc = W.render_call(self.lib, self.be, plan, first_row, nrows, self.be.ptr(buf) + off)
        assert rc == 0, self.lib.rtfe_last_error().decode()
        self.be.sync()
        raw = self.host(buf)
        intact = bool((raw[:off] == 0x5A).all() and (raw[off + nb: off + nb + 64] == 0x5A).all())
        return raw[off: off + nb].copy().view(np.int16).reshape(nrows, plan.params.ntrks), intact


def check(dev, plan, windows=()):
    """the whole tape and the windows, each between guard bytes, against the host renderer"""
    whole = W.render_host(plan)
    for first, n in [(0, plan.total_rows)] + list(windows):
        got, intact = dev.guarded(plan, first, n)
        assert intact, f"rows {first} + {n}: bytes written outside d_rows"
        bad = np.argwhere(got != whole[first: first + n])
        assert bad.size == 0, f"rows {first} + {n}: {len(bad)} samples differ, the first at row {first + bad[0][0]} track {bad[0][1]}: {got[tuple(bad[0])]} for {whole[first + bad[0][0], bad[0][1]]}"
    assert np.array_equal(dev.render(plan), whole)                           # (the public call: render_device)
    return whole


def odd_windows(plan):
    """windows whose first and last bytes leave partial 16-byte vectors (ntrks * 2 bytes a row: an odd row offset does it for every track count but 8 and 16,
    where rows are whole vectors and nothing is partial)"""
    n = plan.total_rows
    return [(1, n - 2), (n // 3 | 1, (n // 3) | 1), (n - 5, 5), (7, 1), (n // 2, 0)]


def mode_case(dev, name, clean=False):
    spec_fn, bits = {"nrzi": (lambda **k: W.nrzi_spec(**k), 8), "nrzi7_even": (lambda **k: W.nrzi_spec(ntrks=7, even=True, **k), 6), "pe": (W.pe_spec, 8),
                     "gcr": (W.gcr_spec, 8)}[name]
    kw = dict(noise_mv=0.0, jitter=0.0) if clean else {}
    spec = spec_fn(seed=3, gap_samples=300, skew_cells=SKEW[:7 if bits == 6 else 9], **kw)
    items = [("mark",), ("block", payload(1, 20, bits, lo=1)), ("block", payload(2, 9, bits, lo=1)), ("mark",)]
    plan = W.encode(items, spec)
    check(dev, plan, odd_windows(plan))


def raw_spec(ntrks, **kw):
    kw.setdefault("gap_samples", 100)
    kw.setdefault("skew_cells", SKEW[:ntrks])
    return W.nrzi_spec(seed=ntrks, ntrks=ntrks, **kw)


def random_masks(seed, nslots, ntrks, density=0.5):
    rng = np.random.default_rng(seed)
    bits = rng.random((nslots, ntrks)) < density
    return (bits * (1 << np.arange(ntrks, dtype=np.uint64))).sum(axis=1).astype(np.uint32)


RAW_NTRKS = (1, 2, 7, 9, 16, 19)


def raw_case(dev, ntrks):
    """random masks (a sign pattern of their own on the second block), three blocks over several spans"""
    flux2 = random_masks(ntrks + 50, 40, ntrks)
    blocks = [(random_masks(ntrks, 30, ntrks), None, 30), (flux2, flux2 & random_masks(ntrks + 60, 40, ntrks), 40.5, 57), (random_masks(ntrks + 70, 3, ntrks, 1.0), None, 3, 1)]
    plan = W.encode_raw(blocks, raw_spec(ntrks))
    check(dev, plan, odd_windows(plan))


def pe_raw_case(dev):
    """half-cell slots outside the PE format: every slot a transition on some track"""
    spec = W.pe_spec(seed=5, gap_samples=90, skew_cells=SKEW[:9])
    plan = W.encode_raw([(random_masks(21, 81, 9, 0.7), None, 41)], spec)
    check(dev, plan, odd_windows(plan))


def seam_case(dev, shift):
    """a block that starts `shift` rows from a span boundary, and one that ends `shift` rows from one (shift -1, 0, 1)"""
    S = dev.span(9)
    spec = raw_spec(9)
    rows = int(W.encode_raw([(random_masks(1, 25, 9), None, 25)], spec).blocks["rows"][0])
    start_a = 2 * S + shift
    end_b = -(-(start_a + 2 * rows + 10) // S) * S + S + shift
    plan = W.encode_raw([(random_masks(1, 25, 9), None, 25, start_a), (random_masks(2, 25, 9), None, 25, end_b - rows - (start_a + rows))], spec)
    assert int(plan.blocks["first_row"][0]) == start_a and int(plan.blocks["first_row"][1] + plan.blocks["rows"][1]) == end_b
    check(dev, plan, [(start_a - 1, 3), (end_b - 2, 3), (S - 1, S + 2)])


def reach_case(dev):
    """lone transitions whose centres lie a few rows either side of span boundaries inside one long block: the pulse reaches across from either side"""
    S = dev.span(9)
    spec = raw_spec(9, gap_samples=10)
    spb, ncells = W.encode_raw([], spec).params.spb, 80
    flux = np.zeros(ncells, np.uint32)
    for boundary in (S, 2 * S, 3 * S):
        for d in (-3, 0, 4):                                                     # the cell whose centre is nearest to boundary + d rows of the tape
            c = int(round((boundary + d - 10) / spb - 8.5))
            flux[c] |= 0x1FF if d else 0x0AA
    plan = W.encode_raw([(flux, None, ncells)], spec)
    assert plan.total_rows > 3 * S + plan.params.K
    check(dev, plan, [(S - 2, 4), (2 * S, 1), (3 * S - 1, 1)])


def short_block_case(dev):
    """blocks shorter than the reach: a pulse wider than its block (K = 24 cells' worth of rows, the block 17)"""
    spec = raw_spec(9, bpi=1600.0, pulse_w=1.5, gap_samples=40)
    plan = W.encode_raw([(np.array([0x1FF], np.uint32), None, 1), (np.array([0x155], np.uint32), np.array([0x101], np.uint32), 1)], spec)
    assert plan.params.K > int(plan.blocks["rows"].max())
    check(dev, plan, odd_windows(plan))


def crowded_case(dev):
    """a span that holds several blocks: 2.5 rows a cell, blocks of 50 rows 10 rows apart"""
    spec = raw_spec(9, bpi=6250.0, gap_samples=10)
    plan = W.encode_raw([(random_masks(k, 4, 9, 0.8), None, 4) for k in range(24)], spec)
    S = dev.span(9)
    assert np.bincount(plan.blocks["first_row"] // S).max() >= 3
    check(dev, plan, odd_windows(plan))


def gaps_case(dev, noise):
    plan = W.encode([], W.nrzi_spec(seed=8, gap_samples=1000, noise_mv=noise))
    assert plan.total_rows == 1000 and plan.blocks.size == 0 and plan.slots.size == 0
    whole = check(dev, plan, odd_windows(plan))
    assert (whole != 0).any() == (noise > 0) and abs(int(whole.max())) < 400


def rails_case(dev):
    """amplitude above maxvolts: both rails, and never the end marker's -32768"""
    spec = W.nrzi_spec(seed=2, gap_samples=200, amplitude=6.0, skew_cells=SKEW[:9])
    plan = W.encode([("block", payload(4, 30))], spec)
    whole = check(dev, plan, odd_windows(plan))
    assert whole.max() == 32767 and whole.min() == -32767


def refusals(dev):
    """every refusal of rtfe_tape_render with its code, and the buffer untouched"""
    plan = W.encode_raw([(random_masks(1, 20, 9), None, 20), (random_masks(2, 20, 9), None, 20)], raw_spec(9))
    be, lib = dev.be, dev.lib
    d_slots, d_blocks = W.device_tables(plan, be)
    n = 64
    buf, off = dev.buffer(n * 9 * 2)
    out = be.ptr(buf) + off

    def call(slots=be.ptr(d_slots), nslots=plan.slots.size, blocks=plan.blocks, d_blk=be.ptr(d_blocks), nblocks=plan.blocks.size, p=plan.params, first=0, nrows=n, rows=out):
        return lib.rtfe_tape_render(slots, nslots, blocks.ctypes.data if blocks is not None else None, d_blk, nblocks, C.byref(p) if p is not None else None,
                                    first, nrows, rows, be.stream())

    def params(**kw):
        p = W.Params.from_buffer_copy(plan.params)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(p, k)[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return p

    def table(**kw):
        t = plan.blocks.copy()
        for k, (i, v) in kw.items():
            t[k][i] = v
        return t

    cases = [(-1, dict(rows=None)), (-1, dict(p=None)), (-1, dict(slots=None)), (-1, dict(blocks=None)), (-1, dict(d_blk=None)),
             (-3, dict(p=params(ntrks=0))), (-3, dict(p=params(ntrks=20))),
             (-31, dict(rows=out + 2)), (-31, dict(rows=out + 8)),
             (-34, dict(nrows=-1)), (-34, dict(first=-1)), (-34, dict(nslots=-1)), (-34, dict(nblocks=-1)), (-34, dict(first=(1 << 63) - 10)),
             (-60, dict(p=params(K=-1))), (-60, dict(p=params(K=2049))), (-60, dict(p=params(spb=0.05))), (-60, dict(p=params(skew=(3, 2000.0)))),
             (-61, dict(blocks=table(first_row=(1, 0)))), (-61, dict(blocks=table(rows=(0, 0)))), (-61, dict(blocks=table(nslots=(1, 21)))),
             (-61, dict(blocks=table(first_slot=(0, -1)))), (-61, dict(blocks=table(rows=(0, int(plan.blocks["first_row"][1]))))),
             (-62, dict(p=params(maxvolts=0.0))), (-62, dict(p=params(spb=float("nan")))), (-62, dict(p=params(w=0.0))), (-62, dict(p=params(pitch_shift=2))),
             (-62, dict(p=params(noise_mv=-1.0))), (-62, dict(p=params(jitter=float("inf")))), (-62, dict(p=params(amp=(8, float("nan")))))]
    for code, kw in cases:
        rc = call(**kw)
        assert rc == code, f"{kw}: {rc} for {code} ({lib.rtfe_last_error().decode()})"
        assert lib.rtfe_last_error().decode().startswith("rtfe_tape_render:")
    be.sync()
    assert (dev.host(buf) == 0x5A).all(), "a refused call wrote"
    assert call(nrows=0) == 0 and call(slots=None, nslots=0, blocks=None, d_blk=None, nblocks=0) == 0          # empty tables need no pointers
    be.sync()
    raw = dev.host(buf)
    assert (raw[:off] == 0x5A).all() and (raw[off + n * 18:] == 0x5A).all() and not (raw[off: off + n * 18] == 0x5A).all()


CASES = {**{f"mode_{m}": (lambda d, m=m: mode_case(d, m)) for m in ("nrzi", "nrzi7_even", "pe", "gcr")},
         **{f"mode_{m}_clean": (lambda d, m=m: mode_case(d, m, clean=True)) for m in ("nrzi", "pe", "gcr")},
         **{f"raw_{n}_tracks": (lambda d, n=n: raw_case(d, n)) for n in RAW_NTRKS},
         "raw_pe_half_cells": pe_raw_case,
         **{f"block_at_span_boundary_{s:+d}": (lambda d, s=s: seam_case(d, s)) for s in (-1, 0, 1)},
         "pulse_reach_across_spans": reach_case, "block_shorter_than_reach": short_block_case, "several_blocks_in_a_span": crowded_case,
         "gaps_only_noise": (lambda d: gaps_case(d, 10.0)), "gaps_only_silent": (lambda d: gaps_case(d, 0.0)), "both_rails": rails_case, "refusals": refusals}


# ---- files ----
def file_case(dev, tmp_path, window_rows=None):
    """write_tbin_device over at least three windows that are no multiple of the span against write_tbin"""
    spec_fn, items, _ = TAPES["nrzi9"]
    plan = W.encode(items[:4], spec_fn())
    S = dev.span(9)
    window_rows = window_rows or (plan.total_rows // 4 // S) * S + 77
    a, b = str(tmp_path / "host.tbin"), str(tmp_path / "device.tbin")
    W.write_tbin(plan, a, window_rows=5001)
    r = W.write_tbin_device(plan, b, window_rows=window_rows, _lib_path=dev.lib_path, _backend=dev.be)
    assert r["windows"] >= 3 and window_rows % S != 0
    data = open(a, "rb").read()
    assert data == open(b, "rb").read() and len(data) == r["bytes"]
    hdr, rows = tbin.read_tbin(a)
    assert (hdr.mode, hdr.bpi, hdr.ips, hdr.ntrks) == (tbin.MODE_NRZI, 800.0, 50.0, 9) and np.array_equal(rows, W.render_host(plan))
    ref = str(tmp_path / "ref.tbin")
    tbin.write_tbin(ref, plan.spec.header(), rows)
    assert data == open(ref, "rb").read()
