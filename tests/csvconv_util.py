"""What the tests of the CSV -> TBIN conversion with window options, -graph and -redo share (csvin.convert_csv / read_csv and their device counterparts):
the goldens' cases and options, the seeded text of the redo recipe, the two loops of the converter restated literally, rtfe_csv_graph called alone and
its numpy restatement.  Test infrastructure."""
import ctypes as C
import dataclasses
import hashlib
import os

import numpy as np

from readtape_amd import csvin, frontend, tbin

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> (lines of text, ntrks, the converter's options); the texts come from make_csvconv_golden.text_for
CASES = {
    "csvconv_graph64": (1500, 9, ["-nrzi", "-graph=64"]),
    "csvconv_skip_stop_graph": (1500, 9, ["-nrzi", "-skip=10", "-stopaft=300", "-graph=64"]),
    "csvconv_sub3_skip_graph7": (1400, 9, ["-nrzi", "-subsample=3", "-skip=10", "-graph=7"]),
    # T0 = 9.99 ms, D = 1 us: K = 210, and the clock gets behind the end time on sample 300, a multiple of the bin - the line "300, ..." is not printed
    "csvconv_start_end_graph100": (1500, 9, ["-nrzi", "-starttime=0.0102", "-endtime=0.0104995", "-graph=100"]),
    "csvconv_start_before_t0": (1200, 9, ["-nrzi", "-starttime=0.011", "-graph=50"]),
    "csvconv_stopaft1": (1000, 9, ["-nrzi", "-stopaft=1", "-graph=1"]),
    "csvconv_order7_invert_scale": (1300, 7, ["-ntrks=7", "-order=543210p", "-invert", "-scale=0.5", "-nrzi", "-graph=33"]),
    "csvconv_graph_bin_too_big": (1000, 9, ["-nrzi", "-graph=5000"]),
}
REDO_LINES = 1000050
REDO_OPTS = ["-ntrks=5", "-nrzi", "-skip=5", "-graph=400000"]


def options(opts):
    """The converter's options -> the keywords of csvin.convert_csv / read_csv."""
    def opt(key, default=None, cast=str):
        for o in opts:
            if o.startswith(key):
                return cast(o[len(key):])
        return default
    mode = tbin.MODE_PE if "-pe" in opts else tbin.MODE_NRZI
    return dict(ntrks=opt("-ntrks=", 9, int), order=opt("-order="), invert="-invert" in opts, scale=opt("-scale=", 1.0, float), subsample=opt("-subsample=", 1, int),
                maxvolts=opt("-maxvolts=", 0.0, float), mode=mode, skip=opt("-skip=", 0, int), starttime=opt("-starttime=", 0.0, float),
                endtime=opt("-endtime=", 0.0, float), stopaft=opt("-stopaft=", None, int), graph=opt("-graph=", 0, int), redo="-redo" in opts)


def load(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    return z, options([str(o) for o in z["opts"]])


def redo_text(nlines=REDO_LINES, seed=11):
    """The redo recipe's file: minimal five-track lines, a microsecond apart, whose last 50 lines exceed the full scale the pre-read (a million lines) arrives at."""
    rng = np.random.RandomState(seed)
    v = rng.randint(-15, 16, size=(nlines, 5))
    v[-50:] = rng.randint(30, 60, size=(50, 5)) * np.where(rng.rand(50, 5) < 0.5, -1, 1)
    t = 1000 + np.arange(nlines)
    out = ["Time [s], a, b, c, d, e", "Time [s], a, b, c, d, e"]
    sign = np.where(v < 0, "-", "")
    a = np.abs(v)
    for i in range(nlines):
        out.append("0.%06d,%s" % (t[i], ",".join("%s%d.%d" % (sign[i, k], a[i, k] // 10, a[i, k] % 10) for k in range(5))))
    return ("\n".join(out) + "\n").encode()


def sha(b):
    return hashlib.sha256(b).hexdigest()


def literal_window(T0, D, nlines, sub, skip, start_ns, end_ns, stopaft):
    """The converter's two loops, line for line, on a file of nlines data lines -> (skipped, first kept raw line or None, kept, ended) or None where
    the file ends inside the skip.  end_ns / stopaft None: not given."""
    end_ns = (1 << 64) - 1 if end_ns is None else end_ns
    stopaft = (1 << 64) - 1 if stopaft is None else stopaft
    pos, clock, skipped = 0, T0, 0                       # pos: raw data lines read so far
    if skip > 0 or start_ns > 0:
        while True:
            if pos >= nlines:
                return None
            pos += 1
            clock += D
            skipped += 1
            if skip > 0:
                skip -= 1
            if not (clock < start_ns or skip > 0):
                break
    first, n, ended = None, 0, "file"
    while True:
        got = True
        for _ in range(sub):
            if pos >= nlines:
                got = False
                break
            pos += 1
        if not got:
            break
        if first is None:
            first = pos - 1
        clock += D
        n += 1
        if n >= stopaft:
            ended = "stopaft"
            break
        if clock > end_ns:
            ended = "endtime"
            break
    return skipped, first, n, ended


# ---- rtfe_csv_graph alone ----
def graph_argtypes(lib):
    lib.rtfe_csv_graph.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_float, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    return lib


def _scan_f32(s, p):
    """csrc/host/rt_csv.c scan_f32 on the bytes s (a line: reading past its end gives NUL) -> (value, p)."""
    f = np.float32
    at = lambda i: s[i] if i < len(s) else 0
    while at(p) in (32, 44):
        p += 1
    neg = at(p) == 45
    if neg:
        p += 1
    v = f(0)
    with np.errstate(all="ignore"):
        while 48 <= at(p) <= 57:
            v = f(f(v * f(10)) + f(at(p) - 48))
            p += 1
        if at(p) == 46:
            p += 1
            scale = f(10)
            while 48 <= at(p) <= 57:
                v = f(v + f(f(at(p) - 48) / scale))
                scale = f(scale * f(10))
                p += 1
    return (-v if neg else v), p


def line_peak(line, ntrks, scale):
    """max_k |field_k * scale| of one line in float32, the time field skipped (the scanners are the same: its value is not used)."""
    _, p = _scan_f32(line, 0)
    peak = np.float32(0)
    for _ in range(ntrks):
        v, p = _scan_f32(line, p)
        v = np.float32(v * np.float32(scale))
        if v < 0:
            v = -v
        if peak < v:
            peak = v
    return peak


def split_lines(text):
    """The lines as rtfe_csv_index cuts them for a last window: each ends behind its newline, an unterminated last line counts."""
    lines = text.split(b"\n")
    out = [ln + b"\n" for ln in lines[:-1]]
    if lines[-1]:
        out.append(lines[-1])
    return out


def graph_reference(lines, first_line, step, nkept, ntrks, scale, first_sample, graphbin, bins, peak):
    """rtfe_csv_graph in numpy on the bins (float32, updated in place) -> the new peak."""
    for j in range(nkept):
        v = line_peak(lines[first_line + j * step], ntrks, scale)
        b = (first_sample + j) // graphbin
        if b < len(bins) and v > bins[b]:
            bins[b] = v
        if v > peak:
            peak = v
    return peak


class Graph:
    """rtfe_csv_index + rtfe_csv_graph on a backend's memory, with guard words behind the bins."""

    def __init__(self, be, lib_path=None):
        self.be, self.lib = be, graph_argtypes(frontend._load_library(lib_path))
        self.dev = csvin._Dev(be, False)

    def index(self, text):
        be, lib, dev = self.be, self.lib, self.dev
        d_text = dev.alloc(len(text) + 16)
        dev.zero(d_text)
        be.upload(d_text, text)
        cap = text.count(b"\n") + 2
        d_starts = dev.alloc(4 * (cap + 1))
        scratch = dev.alloc(lib.rtfe_csv_index_scratch_bytes(len(text)))
        out = dev.alloc(32)
        assert lib.rtfe_csv_index(be.ptr(d_text), len(text), 1, be.ptr(d_starts), cap, be.ptr(scratch), int(scratch.shape[0]), be.ptr(out), be.stream()) == 0
        return d_text, d_starts

    def buffers(self, nbins, values=None):
        """nbins float32 bins (zero, or `values`) with 16 guard words behind them, and a peak word."""
        d = self.dev.alloc(4 * (nbins + 16) + 16)
        init = np.zeros(nbins + 16, dtype=np.float32)
        if values is not None:
            init[:nbins] = values
        init[nbins:] = np.float32(12345.0)
        self.be.upload(d, init.tobytes())
        d_peak = self.dev.alloc(16)
        self.dev.zero(d_peak)
        return d, d_peak

    def run(self, d_text, d_starts, first_line, step, nkept, ntrks, scale, first_sample, graphbin, d_bins, nbins, d_peak):
        be = self.be
        return self.lib.rtfe_csv_graph(be.ptr(d_text), be.ptr(d_starts), first_line, step, nkept, ntrks, scale, first_sample, graphbin,
                                       be.ptr(d_bins) if d_bins is not None else None, nbins, be.ptr(d_peak) if d_peak is not None else None, be.stream())

    def read(self, d_bins, nbins, d_peak):
        self.be.sync()
        a = np.array(self.be.to_numpy(d_bins[: 4 * (nbins + 16)], np.float32)[: nbins + 16])
        assert np.all(a[nbins:] == np.float32(12345.0)), "rtfe_csv_graph wrote at or behind d_bins + nbins"
        pk = None if d_peak is None else np.array(self.be.to_numpy(d_peak[:4], np.float32))[0]
        return a[:nbins], pk


def fields_text(nlines, ntrks, seed, digits=6, amp=3.0, peak_at=None, tail_newline=True):
    """nlines data lines "time, v0, ..." of `digits` decimals; peak_at = (line, value): that line's first field."""
    rng = np.random.RandomState(seed)
    v = rng.uniform(-amp, amp, (nlines, ntrks))
    if peak_at is not None:
        v[peak_at[0], 0] = peak_at[1]
    text = b"".join((f"{0.0125 + i * 1.28e-6:.9f}, " + ", ".join(f"{x:.{digits}f}" for x in v[i]) + "\n").encode() for i in range(nlines))
    return text if tail_newline else text[:-1]


def graph_cases():
    """(name, text, calls, ntrks, scale, nbins or None = what the lines need): calls = [(first_line, step, nkept, first_sample, graphbin)], all on one
    pair of buffers; nbins "short" = one less than needed."""
    out = []
    t9 = fields_text(300, 9, 1)
    for gb in (1, 2, 63, 64, 65, 128, 1000, 5000):
        out.append((f"bin{gb}", t9, [(0, 1, 300, 0, gb)], 9, 1.0, None))
    out.append(("first_sample_odd", t9, [(0, 1, 300, 37, 64)], 9, 1.0, None))
    out.append(("two_calls_one_bin", t9, [(0, 1, 100, 0, 64), (100, 1, 200, 100, 64)], 9, 1.0, None))
    out.append(("two_calls_one_bin_step3", t9, [(2, 3, 30, 0, 7), (92, 3, 60, 30, 7)], 9, 0.5, None))
    out.append(("step3", t9, [(2, 3, 99, 0, 10)], 9, 1.0, None))
    out.append(("wide19", fields_text(200, 19, 2, digits=14), [(0, 1, 200, 5, 64)], 19, 1.0, None))      # 19 fields of 17 bytes: a wave's 64 lines are 21 KB
    for n in (1, 5, 9, 19):
        out.append((f"ntrks{n}", fields_text(150, n, 3 + n), [(0, 1, 150, 0, 64)], n, 2.0, None))
    out.append(("max_lane0", fields_text(192, 9, 4, peak_at=(64, -7.5)), [(0, 1, 192, 0, 64)], 9, 1.0, None))
    out.append(("max_lane63", fields_text(192, 9, 4, peak_at=(127, 7.5)), [(0, 1, 192, 0, 64)], 9, 1.0, None))
    odd = b"0.001, -0.0, -0.0\n0.002, 1.5\n0.003\n\n0.005, -0.0, 2.5, 9.9\n0.006, -3.25, 1"          # minus zero, missing fields, a blank line, no last newline
    out.append(("odd_lines", odd, [(0, 1, 6, 0, 2)], 2, 1.0, None))
    out.append(("unterminated", fields_text(70, 5, 9, tail_newline=False), [(0, 1, 70, 0, 64)], 5, 1.0, None))
    out.append(("nbins_short", t9, [(0, 1, 300, 0, 64)], 9, 1.0, "short"))
    out.append(("nbins_short_bin1", t9, [(0, 1, 300, 0, 1)], 9, 1.0, "short"))
    out.append(("nbins_zero", t9, [(0, 1, 300, 0, 64)], 9, 1.0, 0))
    return out


def run_graph_case(g, case, with_peak=True):
    name, text, calls, ntrks, scale, nbins = case
    lines = split_lines(text)
    need = max((fs + nk - 1) // gb + 1 for _, _, nk, fs, gb in calls)
    nbins = need if nbins is None else (need - 1 if nbins == "short" else nbins)
    d_text, d_starts = g.index(text)
    start = np.linspace(0.0, 0.5, nbins).astype(np.float32) if name.startswith("two_calls") else None      # (old values stay where they are larger)
    d_bins, d_peak = g.buffers(nbins, start)
    want = np.zeros(nbins, dtype=np.float32) if start is None else start.copy()
    peak = np.float32(0)
    for first_line, step, nkept, first_sample, gb in calls:
        rc = g.run(d_text, d_starts, first_line, step, nkept, ntrks, scale, first_sample, gb, d_bins, nbins, d_peak if with_peak else None)
        assert rc == 0, (name, rc, g.lib.rtfe_last_error())
        peak = graph_reference(lines, first_line, step, nkept, ntrks, scale, first_sample, gb, want, peak)
    got, pk = g.read(d_bins, nbins, d_peak if with_peak else None)
    assert got.tobytes() == want.tobytes(), (name, np.flatnonzero(got != want)[:5], got[:4], want[:4])
    if with_peak:
        assert pk.tobytes() == np.float32(peak).tobytes(), (name, pk, peak)


def run_graph_refusals(g):
    text = fields_text(4, 2, 1)
    d_text, d_starts = g.index(text)
    d_bins, d_peak = g.buffers(4)
    run, err = g.run, g.lib.rtfe_last_error
    assert run(d_text, d_starts, 0, 1, 4, 2, 1.0, 0, 0, d_bins, 4, d_peak) == -34 and b"graphbin" in err()
    assert run(d_text, d_starts, 0, 1, 4, 2, 1.0, 0, 1, d_bins, -1, d_peak) == -34 and b"nbins" in err()
    assert run(d_text, d_starts, 0, 1, 4, 0, 1.0, 0, 1, d_bins, 4, d_peak) == -3
    assert run(d_text, d_starts, 0, 1, 4, 20, 1.0, 0, 1, d_bins, 4, d_peak) == -3
    assert run(d_text, d_starts, 0, 0, 4, 2, 1.0, 0, 1, d_bins, 4, d_peak) == -34
    assert run(d_text, d_starts, -1, 1, 4, 2, 1.0, 0, 1, d_bins, 4, d_peak) == -34
    assert run(d_text, d_starts, 0, 1, 4, 2, 1.0, -1, 1, d_bins, 4, d_peak) == -34
    assert run(d_text, d_starts, 0, 1, 4, 2, 1.0, 0, 1, None, 4, d_peak) == -1
    assert run(d_text[4:], d_starts, 0, 1, 4, 2, 1.0, 0, 1, d_bins, 4, d_peak) == -31
    assert run(d_text, d_starts, 0, 1, 0, 2, 1.0, 0, 1, d_bins, 4, d_peak) == 0
    got, pk = g.read(d_bins, 4, d_peak)
    assert not got.any() and pk == 0
    assert g.lib.rtfe_abi_version() == 6 and g.lib.rtfe_kernel_count() == 12


# ---- the device conversion against the host's ----
def same_info(tag, got, want):
    for k in ("clipped_samples", "columns", "skipped", "samples", "too_big", "too_small", "redone", "ended"):
        assert got[k] == want[k], (tag, k, got[k], want[k])
    assert ("graph" in got) == ("graph" in want), tag
    if "graph" in want:
        assert np.array_equal(got["graph"][0], want["graph"][0]) and got["graph"][1].tobytes() == want["graph"][1].tobytes(), (tag, got["graph"], want["graph"])


def check_device_equals_host(tag, text, kw, tmp_path, be, lib_path, windows=(4096, 1 << 28), preread=None, path="device"):
    """read_csv_device == read_csv and convert_csv_device == convert_csv (both files' bytes) for one text and one set of options."""
    from csv_device_util import host_rows
    src = str(tmp_path / "c.csv")
    open(src, "wb").write(text)
    times = tuple(range(1, 28))
    try:
        want = csvin.read_csv(src, _preread_rows=preread, **kw)
    except ValueError:
        want = None
    for w in windows:
        if want is None:
            for f in (lambda: csvin.read_csv_device(src, window_bytes=w, _lib_path=lib_path, _backend=be, _preread_rows=preread, **kw),
                      lambda: csvin.convert_csv_device(src, str(tmp_path / "d.tbin"), window_bytes=w, _lib_path=lib_path, _backend=be, _preread_rows=preread, **kw)):
                try:
                    f()
                except ValueError:
                    continue
                raise AssertionError(f"{tag}: the host refuses these options for this file, the device path does not")
            continue
        hdr, rows, info = csvin.read_csv_device(src, window_bytes=w, _lib_path=lib_path, _backend=be, _preread_rows=preread, **kw)
        t = f"{tag} window_bytes={w}"
        assert info["path"] == path, (t, info)
        assert hdr == want[0], (t, hdr, want[0])
        got = host_rows(be, rows)
        assert got.shape == want[1].shape and np.array_equal(got, want[1]), (t, got.shape, want[1].shape)
        same_info(t, info, want[2])
        a, b = str(tmp_path / "h.tbin"), str(tmp_path / "d.tbin")
        for p in (a, b, a[:-5] + ".graph.csv", b[:-5] + ".graph.csv"):
            if os.path.exists(p):
                os.remove(p)
        hh, hi = csvin.convert_csv(src, a, times=times, _preread_rows=preread, **kw)
        dh, di = csvin.convert_csv_device(src, b, times=times, window_bytes=w, _lib_path=lib_path, _backend=be, _preread_rows=preread, **kw)
        assert dh == hh and di["path"] == path, (t, dh, hh, di)
        same_info(t + " files", di, hi)
        assert open(a, "rb").read() == open(b, "rb").read(), t
        assert open(a, "rb").read() == tbin.pack_header(dataclasses.replace(want[0], times=times)) + want[1].tobytes() + b"\x00\x80", t
        ga, gb = a[:-5] + ".graph.csv", b[:-5] + ".graph.csv"
        assert os.path.exists(ga) == os.path.exists(gb) == bool(kw.get("graph")), t
        if kw.get("graph"):
            assert open(ga, "rb").read() == open(gb, "rb").read(), t
    return want


def device_option_sets():
    """Window options to run csv_shapes' shapes with: skips and stops that straddle small windows, bins of 1, 7 and 64, a time window."""
    return [dict(skip=3, graph=7), dict(skip=17, stopaft=21, graph=1), dict(stopaft=40, graph=64, redo=True), dict(starttime=0.01251, endtime=0.01255, graph=5),
            dict(skip=1000000)]
