"""What the host, the emulated and the GPU tests of the CSV export (readtape_amd/csvout.py; kernels in readtape_amd/csrc/rtfe_csvout.hip) share: the goldens
made by tests/make_csvout_golden.py from the reference converter's -read, the Python model of its text, and the cases the device path is run through - every
one a comparison of bytes with the host writer write_csv (fprintf), which the goldens pin to the reference.  Test infrastructure."""
import ctypes as C
import glob
import os

import numpy as np

from readtape_amd import csvin, csvout, frontend, tbin

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = sorted(os.path.basename(p)[len("csvout_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "csvout_*.npz")))
EXPECTED_GOLDENS = ["endmark_mid", "inv_ties", "order7", "plain9", "rail_col", "rail_col_inv", "stagger15", "stagger_ties", "t10000", "win_endtime", "win_skip",
                    "win_skip_starttime", "win_skip_stop_end", "win_start_end", "win_starttime", "win_stopaft"]
# the goldens whose rows come back from the reference's own text through read_csv (test_csvout_host checks that they do): modest amplitudes (a full
# scale derived from the text's peak must not exceed the header's), no stagger, no window option
ROUNDTRIP = ["plain9", "inv_ties", "order7"]
WINDOW_ROWS = (1, 63, 64, 65, 1000)


def load_golden(name):
    """-> (header, rows as the file holds them - the end mark's row and what follows included -, write_csv's keywords, the reference's text)."""
    z = np.load(os.path.join(GOLDEN, f"csvout_{name}.npz"))
    raw = z["tbin"].tobytes()
    hdr, off = tbin.parse_header(raw[:4096])
    payload = np.frombuffer(raw, dtype="<i2", offset=off)
    rows = payload[: payload.size // hdr.ntrks * hdr.ntrks].reshape(-1, hdr.ntrks)
    kw = {}
    for o in (str(o) for o in z["opts"]):
        key, val = o[1:].split("=")
        if key == "order":
            kw["order"] = val
        elif key in ("stagger", "starttime", "endtime"):
            kw[key] = float(val)
        elif key in ("skip", "stopaft"):
            kw[key] = int(val)
        else:
            assert key == "ntrks"
    return hdr, rows, kw, z["csv"].tobytes()


def model_text(hdr, rows, order=None, stagger=0.0, **window):
    """The reference's text by Python's % (correctly rounded, like glibc's printf) and numpy's float32."""
    ends = np.flatnonzero(rows[:, 0] == tbin.END_MARK)
    n = int(ends[0]) if ends.size else rows.shape[0]
    first, count = csvout.export_window(hdr, n, **window)
    perm = frontend.parse_track_order(order) if order else list(range(hdr.ntrks))
    out = [csvout.title_lines(hdr)]
    mv, st = np.float32(hdr.maxvolts), np.float32(stagger)
    for r in range(first, first + count):
        line = "%12.8f, " % ((hdr.tstart_ns + r * hdr.tdelta_ns) / 1e9)
        amount = np.float32(0)
        for k in range(hdr.ntrks):
            f = np.float32(rows[r, perm[k]]) / np.float32(32767) * mv
            if hdr.flags & tbin.FLAG_INVERTED:
                f = -f
            f = np.float32(f + amount)
            amount = np.float32(amount + st)
            line += "%9.5f, " % float(f)
        out.append(line.encode() + b"\n")
    return b"".join(out)


def host_text(tmp_path, hdr, rows, **kw):
    path = str(tmp_path / "host.csv")
    info = csvout.write_csv(path, hdr, rows, **kw)
    text = open(path, "rb").read()
    assert info["bytes"] == len(text)
    return text, info


def device_text(tmp_path, be, lib_path, hdr, rows, **kw):
    path = str(tmp_path / "device.csv")
    info = csvout.write_csv_device(path, hdr, rows, _lib_path=lib_path, _backend=be, **kw)
    text = open(path, "rb").read()
    assert info["bytes"] == len(text) and info["rows"] == text.count(b"\n") - 2
    return text, info


def first_difference(got, want):
    if got == want:
        return None
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return (i, a, b)
    return (min(len(g), len(w)), len(got), len(want))


def same(got, want, tag):
    assert got == want, (tag, first_difference(got, want))


def hdr_for(ntrks=9, tdelta=1000, maxvolts=1.0, invert=False, tstart=1_000_000):
    return tbin.TbinHeader(ntrks=ntrks, tdelta_ns=tdelta, maxvolts=maxvolts, mode=tbin.MODE_NRZI, bpi=800.0, ips=50.0,
                           flags=tbin.FLAG_NO_REORDER | (tbin.FLAG_INVERTED if invert else 0), tstart_ns=tstart, descr="t")


def check_against_host(tmp_path, be, lib_path, hdr, rows, path=None, tag="", **kw):
    """write_csv_device == write_csv, and the layout it took."""
    want, _ = host_text(tmp_path, hdr, rows, **{k: v for k, v in kw.items() if k != "window_rows"})
    got, info = device_text(tmp_path, be, lib_path, hdr, rows, **kw)
    same(got, want, tag)
    if path is not None:
        assert info["path"] == path, (tag, info)
    return info


# ---- the cases ----
def run_golden(name, tmp_path, be, lib_path=None):
    """A golden through write_csv_device is the reference's text: whole, and in windows that cut it in front of, on and behind a wave's 64 rows."""
    hdr, rows, kw, want = load_golden(name)
    got, info = device_text(tmp_path, be, lib_path, hdr, rows, **kw)
    same(got, want, name)
    assert info["windows"] <= 1
    for w in WINDOW_ROWS:
        got, info = device_text(tmp_path, be, lib_path, hdr, rows, window_rows=w, **kw)
        same(got, want, (name, w))
        assert info["windows"] == -(-info["rows"] // w)


def every_code_rows():
    """7282 rows of nine tracks that hold every int16 value, column 0 never the end mark (65536 = 7281 * 9 + 7: the last row is filled up with zeros;
    the one -32768 that falls into column 0 changes places with its neighbour)."""
    codes = np.arange(-32768, 32768, dtype=np.int32)
    codes = np.concatenate([codes[1:2], codes[0:1], codes[2:], np.zeros(7282 * 9 - 65536, np.int32)]).astype(np.int16)
    rows = codes.reshape(7282, 9)
    assert not (rows[:, 0] == -32768).any() and np.unique(rows).size == 65536
    return rows


EVERY_CODE = [(mv, inv) for mv in (0.1, 1.0, 3.3, 5.0, 15.0) for inv in (False, True)]


def run_every_code(mv, inv, tmp_path, be, lib_path=None):
    """Every int16 code at one full scale: the plain tapes from 1 ms (the uniform layout), the inverted ones from 2000 s (the general one)."""
    hdr = hdr_for(maxvolts=mv, invert=inv, tstart=2_000_000_000_000 if inv else 1_000_000)
    check_against_host(tmp_path, be, lib_path, hdr, every_code_rows(), path="general" if inv else "uniform", tag=(mv, inv), window_rows=4000)


def run_ntrks(ntrks, tmp_path, be, lib_path=None):
    """130 rows of 1 .. 19 tracks: the uniform line is 14 + 11 ntrks + 1 bytes - every residue mod 16 -; then the same rows with lines of many lengths."""
    rng = np.random.RandomState(ntrks)
    rows = rng.randint(-32767, 32768, (130, ntrks)).astype(np.int16)
    check_against_host(tmp_path, be, lib_path, hdr_for(ntrks=ntrks, maxvolts=3.3), rows, path="uniform", tag=ntrks)
    check_against_host(tmp_path, be, lib_path, hdr_for(ntrks=ntrks, maxvolts=3.3), rows, path="uniform", tag=ntrks, window_rows=67)
    check_against_host(tmp_path, be, lib_path, hdr_for(ntrks=ntrks, maxvolts=15.0, tstart=999_999_950_000, tdelta=1285), rows, path="general", tag=ntrks, stagger=47.3)
    check_against_host(tmp_path, be, lib_path, hdr_for(ntrks=ntrks, maxvolts=15.0, tstart=999_999_950_000, tdelta=1285), rows, tag=ntrks, stagger=47.3, window_rows=33)


def run_voltage_width_seams(tmp_path, be, lib_path=None):
    """A field grows to 10 characters at -100.00000 and at 1000.00000.  float32 is coarser than five decimals there (its neighbours of 100 are 7.6e-6 apart,
    of 1000 6.1e-5), so no value ROUNDS across either seam: the seams are the exact values, reached here by the stagger on zero rows and by the rail codes at
    a full scale of exactly 100 and 1000 volts, each beside its float32 neighbour on the short side."""
    zero = np.zeros((70, 6), np.int16)
    below = lambda x: float(np.nextafter(np.float32(x), np.float32(0)))
    for st in (-50.0, below(-50.0), -33.333332, 500.0, below(500.0), 333.33334, 99.5, -9.9999999):
        path = "general" if 32768 / 32767 + 5 * abs(st) >= 99 else "uniform"
        check_against_host(tmp_path, be, lib_path, hdr_for(ntrks=6), zero, path=path, tag=("stagger", st), stagger=st)
    rails = np.tile(np.array([[32767, -32767, -32768, 32766, -32766, 1]], np.int16), (70, 1))
    rails[:, 0] = 32767
    for mv in (100.0, below(100.0), 1000.0, below(1000.0), 99.99, 10.0):
        for inv in (False, True):
            check_against_host(tmp_path, be, lib_path, hdr_for(ntrks=6, maxvolts=mv, invert=inv), rails, path="general" if mv > 98 else "uniform", tag=("rails", mv, inv))


def run_time_width_seams(tmp_path, be, lib_path=None):
    """The time field grows at 1000 s and at 10000 s - where the time ROUNDS to it, 5 ns early: the first long line is row 0, 1, 63, 64 and the last row of
    a window of 130 rows; a window with a single long line is general, the one before it uniform."""
    rng = np.random.RandomState(11)
    rows = rng.randint(-32767, 32768, (260, 9)).astype(np.int16)
    for seam in (10 ** 12, 10 ** 13):
        for r in (0, 1, 63, 64, 129):
            hdr = hdr_for(tdelta=7, tstart=seam - 5 - 7 * r)
            info = check_against_host(tmp_path, be, lib_path, hdr, rows[:130], path="general", tag=(seam, r), window_rows=130)
            assert info["windows"] == 1
    # rows 0 .. 129 short, row 130 + 129 the first long one: the first window is uniform, the second has one long line
    hdr = hdr_for(tdelta=7, tstart=10 ** 12 - 5 - 7 * 259)
    assert check_against_host(tmp_path, be, lib_path, hdr, rows, path="mixed", tag="mixed", window_rows=130)["windows"] == 2
    assert check_against_host(tmp_path, be, lib_path, hdr, rows[:130], path="uniform", tag="short", window_rows=130)["windows"] == 1
    assert check_against_host(tmp_path, be, lib_path, hdr, rows, path="general", tag="one window")["windows"] == 1
    # (the time 4 ns in front of the seam still rounds down: uniform)
    check_against_host(tmp_path, be, lib_path, hdr_for(tdelta=1, tstart=10 ** 12 - 6 - 129), rows[:130], path="uniform", tag="just short")


def run_time_ties(tmp_path, be, lib_path=None):
    rng = np.random.RandomState(12)
    rows = rng.randint(-32767, 32768, (300, 9)).astype(np.int16)
    # every row's time an exact tie of the double: (2 i + 1) / 512 s
    hdr = hdr_for(tdelta=3906250, tstart=1953125)
    check_against_host(tmp_path, be, lib_path, hdr, rows, path="uniform", tag="true ties")
    got, _ = device_text(tmp_path, be, lib_path, hdr, rows[:2])
    assert got.split(b"\n")[2].startswith(b"  0.00195312, ") and got.split(b"\n")[3].startswith(b"  0.00585938, ")
    # ties of the ninth decimal that the double resolves one way or the other
    check_against_host(tmp_path, be, lib_path, hdr_for(tdelta=1285, tstart=1_000_000), rows, path="uniform", tag="1285")
    check_against_host(tmp_path, be, lib_path, hdr_for(tdelta=1285, tstart=5), rows, path="uniform", tag="1285 from 5")
    check_against_host(tmp_path, be, lib_path, hdr_for(tdelta=10, tstart=123_456_789_005), rows, path="uniform", tag="all fives")
    check_against_host(tmp_path, be, lib_path, hdr_for(tdelta=4_000_000_010, tstart=400_000_000_000_005), rows[:35], path="general", tag="all fives, days")
    # the last time the device path takes, 2^49 - 1 ns; one more is refused
    last = hdr_for(tdelta=1, tstart=(1 << 49) - 100)
    check_against_host(tmp_path, be, lib_path, last, rows[:100], path="general", tag="2^49 - 1")
    try:
        device_text(tmp_path, be, lib_path, last, rows[:101])
    except ValueError as e:
        assert "-47" in str(e), e
    else:
        raise AssertionError("a window that ends at 2^49 ns was not refused")


class Format:
    """rtfe_csv_format alone on a backend's memory, 64 canary bytes behind text_cap."""

    def __init__(self, be, lib_path=None):
        self.be, self.lib = be, frontend._load_library(lib_path)

    def __call__(self, hdr, rows, first, n, text_cap, stagger=0.0, order=None, misalign=0, scratch_short=0, args=None):
        be, lib = self.be, self.lib
        dev = csvin._Dev(be, False)
        d_rows = be.rows(rows)
        a = args or csvout.format_args(hdr, order, stagger)
        d_text = dev.alloc(text_cap + 64 + 16)
        canary = bytes(range(101, 165))
        be.upload(d_text[text_cap:], canary)
        scratch = dev.alloc(lib.rtfe_csv_format_scratch_bytes(n))
        out = dev.alloc(32)
        rc = lib.rtfe_csv_format(be.ptr(d_rows), first, n, C.byref(a), be.ptr(d_text) + misalign, text_cap, be.ptr(scratch), lib.rtfe_csv_format_scratch_bytes(n) - scratch_short,
                                 be.ptr(out), be.stream())
        if rc != 0:
            return rc, lib.rtfe_last_error().decode(), None
        be.sync()
        o = csvout._Text.from_buffer_copy(bytes(be.to_numpy(out[:24], np.uint8)))
        got = bytes(be.to_numpy(d_text[: text_cap + 64], np.uint8)[: text_cap + 64])
        assert got[text_cap:] == canary, "rtfe_csv_format wrote behind text_cap"
        return 0, o, got[:text_cap]


def run_bounds(tmp_path, fmt):
    """A text that does not fit: the flag, the full byte count, the bytes that fit, nothing behind the cap (Format checks the canary) - on both layouts."""
    rng = np.random.RandomState(13)
    rows = rng.randint(-32767, 32768, (200, 9)).astype(np.int16)
    for hdr, uniform in ((hdr_for(), True), (hdr_for(tstart=999_999_900_000, tdelta=1285), False)):
        want, _ = host_text(tmp_path, hdr, rows)
        body = want[len(csvout.title_lines(hdr)):]
        lines = body.split(b"\n")[:-1]
        part = b"".join(ln + b"\n" for ln in lines[7: 7 + 150])                   # rows 7 .. 156
        longest = max(len(ln) + 1 for ln in lines[7: 7 + 150])
        assert fmt.lib.rtfe_csv_format_path(7, 150, C.byref(csvout.format_args(hdr))) == (1 if uniform else 0)
        for cap in (len(part) + 100, len(part), len(part) - (len(lines[156]) + 1), len(part) - 7, 16 * 64 + 3, 1, 0):
            rc, o, got = fmt(hdr, rows, 7, 150, cap)
            assert rc == 0, o
            assert (o.bytes, o.rows, o.longest) == (len(part), 150, longest), (cap, o.bytes, o.rows, o.longest)
            assert o.flags == (csvout.CSV_TEXT_FULL if cap < len(part) else 0), (cap, o.flags)
            assert got[: min(cap, len(part))] == part[:cap], (uniform, cap)
        assert len(part) <= fmt.lib.rtfe_csv_format_max_bytes(150, 9)
    rc, o, got = fmt(hdr_for(), rows, 5, 0, 64)                                    # an empty window
    assert rc == 0 and (o.bytes, o.rows, o.flags, o.longest) == (0, 0, 0, 0)


def run_refusals(fmt):
    lib = fmt.lib
    rows = np.zeros((10, 9), np.int16)
    code = lambda *a, **k: fmt(*a, **k)[:2]
    assert code(hdr_for(ntrks=9), rows, 0, 10, 4096, misalign=4)[0] == -31
    assert code(hdr_for(ntrks=9), rows, 0, 10, 4096, scratch_short=1)[0] == -32
    assert code(hdr_for(ntrks=9), rows, -1, 10, 4096)[0] == -34 and code(hdr_for(ntrks=9), rows, 0, -1, 4096)[0] == -34
    for n in (0, 20):
        a = csvout._FormatArgs(n, 0, 1.0, 0.0, 0, 1000, None)
        rc, msg = code(None, rows, 0, 10, 4096, args=a)
        assert rc == -3 and "ntrks" in msg
    perm = (C.c_int * 3)(0, 3, 1)
    a = csvout._FormatArgs(3, 0, 1.0, 0.0, 0, 1000, C.cast(perm, C.POINTER(C.c_int)))
    rc, msg = code(None, np.zeros((10, 3), np.int16), 0, 10, 4096, args=a)
    assert rc == -4 and "perm[1]" in msg
    # the voltage domain: |maxvolts| 32768 / 32767 + (ntrks - 1) |stagger| below 2^20, and finite
    for mv, st in ((1048576.0, 0.0), (1.0, 131072.0), (float("inf"), 0.0), (1.0, float("nan")), (-1048576.0, 0.0)):
        a = csvout._FormatArgs(9, 0, mv, st, 0, 1000, None)
        rc, msg = code(None, rows, 0, 10, 4096, args=a)
        assert rc == -46 and "domain" in msg, (mv, st, rc)
    assert code(None, rows, 0, 10, 4096, args=csvout._FormatArgs(9, 0, 1048000.0, 0.0, 0, 1000, None))[0] == 0
    # the time domain: the window's last time below 2^49 ns
    assert code(hdr_for(tstart=(1 << 49) - 9, tdelta=1), rows, 0, 10, 4096)[0] == -47
    assert code(hdr_for(tstart=(1 << 49) - 10, tdelta=1), rows, 0, 10, 4096)[0] == 0
    assert code(hdr_for(tstart=0, tdelta=0xFFFFFFFF), rows, 1 << 40, 0, 4096)[0] == 0      # (no row, no time)
    assert lib.rtfe_csv_format_path(0, 10, C.byref(csvout._FormatArgs(20, 0, 1.0, 0.0, 0, 1000, None))) == -3
    assert lib.rtfe_abi_version() == 6 and lib.rtfe_kernel_count() == 12


def run_round_trip(name, tmp_path, be, lib_path=None):
    """rows -> write_csv_device -> read_csv_device (the header's full scale and inversion, the same -order=) -> the rows."""
    hdr, rows, kw, _ = load_golden(name)
    assert set(kw) <= {"order"}
    path = str(tmp_path / "rt.csv")
    csvout.write_csv_device(path, hdr, rows, _lib_path=lib_path, _backend=be, **kw)
    hdr2, rows2, info = csvin.read_csv_device(path, ntrks=hdr.ntrks, mode=hdr.mode, bpi=hdr.bpi, ips=hdr.ips, maxvolts=hdr.maxvolts,
                                              invert=bool(hdr.flags & tbin.FLAG_INVERTED), _lib_path=lib_path, _backend=be, **kw)
    got = rows2 if isinstance(rows2, np.ndarray) else rows2.cpu().numpy()
    assert info["path"] == "device" and np.float32(hdr2.maxvolts) == np.float32(hdr.maxvolts)
    assert got.shape == rows.shape and np.array_equal(got, rows), np.argwhere(got != rows)[:5]
    assert hdr2.tdelta_ns == hdr.tdelta_ns
