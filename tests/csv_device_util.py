"""What the emulated and the GPU tests of the device CSV path (csvin.read_csv_device) share: the comparison with the host loader, the goldens'
options, rtfe_csv_index called alone.  Test infrastructure."""
import os

import numpy as np

from readtape_amd import csvin, frontend, tbin

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CSV_CASES = ["csv_nrzi9", "csv_nrzi7_order_sub2", "csv_pe_scale", "csv_nrzi7_order_late"]


def host_rows(be, rows):
    """The rows of read_csv_device on the host, whatever the backend."""
    if isinstance(rows, np.ndarray):
        return rows
    return rows.cpu().numpy()


def check_shape(sh, tmp_path, be, lib_path=None):
    """read_csv_device == read_csv for one shape of csv_shapes, at each of its window sizes: header, rows, clipped_samples, columns; the path it took."""
    path = str(tmp_path / (sh["name"] + ".csv"))
    open(path, "wb").write(sh["text"])
    try:
        want = csvin.read_csv(path, _preread_rows=sh["preread"], **sh["kw"])
    except OSError as e:
        want = e
    for w in sh["windows"]:
        if isinstance(want, OSError):
            try:
                csvin.read_csv_device(path, window_bytes=w, _lib_path=lib_path, _backend=be, _preread_rows=sh["preread"], **sh["kw"])
            except OSError:
                continue
            raise AssertionError(f"{sh['name']}: the host loader refuses the file, the device path does not")
        hdr, rows, info = csvin.read_csv_device(path, window_bytes=w, _lib_path=lib_path, _backend=be, _preread_rows=sh["preread"], **sh["kw"])
        tag = f"{sh['name']} window_bytes={w}"
        assert info["path"] == sh["path"], (tag, info)
        assert hdr == want[0], (tag, hdr, want[0])
        got = host_rows(be, rows)
        assert got.dtype == np.int16 and got.shape == want[1].shape, (tag, got.shape, want[1].shape)
        assert np.array_equal(got, want[1]), (tag, np.argwhere(got != want[1])[:5])
        assert (info["clipped_samples"], info["columns"]) == (want[2]["clipped_samples"], want[2]["columns"]), (tag, info, want[2])
        ptr = rows.ctypes.data if isinstance(rows, np.ndarray) else rows.data_ptr()
        assert ptr % 16 == 0 and (rows.flags["C_CONTIGUOUS"] if isinstance(rows, np.ndarray) else rows.is_contiguous()), tag
    return want


def golden_options(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    opts, dopts = [str(o) for o in z["opts"]], [str(o) for o in z["decode_opts"]]

    def opt(src, key, default=None, cast=str):
        for o in src:
            if o.startswith(key):
                return cast(o[len(key):])
        return default
    want_hdr, off = tbin.parse_header(z["tbin"].tobytes()[:4096])
    kw = dict(ntrks=opt(opts, "-ntrks=", 9, int), order=opt(opts, "-order="), invert="-invert" in opts, scale=opt(opts, "-scale=", 1.0, float),
              subsample=opt(opts, "-subsample=", 1, int), maxvolts=opt(opts, "-maxvolts=", 0.0, float), mode=want_hdr.mode, bpi=want_hdr.bpi, ips=want_hdr.ips)
    return z, kw, want_hdr, off, opt(dopts, "-order=")


def check_golden_tbin(name, tmp_path, be, lib_path=None, window_bytes=1 << 28):
    """A golden CSV through read_csv_device is the converter's .tbin: header fields, flags, every code."""
    z, kw, want_hdr, off, _ = golden_options(name)
    path = str(tmp_path / "c.csv")
    open(path, "wb").write(z["csv"].tobytes())
    want = np.frombuffer(z["tbin"].tobytes(), dtype="<i2", offset=off)
    want_rows = want[:-1].reshape(-1, kw["ntrks"])
    hdr, rows, info = csvin.read_csv_device(path, window_bytes=window_bytes, _lib_path=lib_path, _backend=be, **kw)
    assert info["path"] == "device" and info["columns"] == kw["ntrks"]
    assert (hdr.tdelta_ns, hdr.tstart_ns, hdr.ntrks) == (want_hdr.tdelta_ns, want_hdr.tstart_ns, want_hdr.ntrks)
    assert np.float32(hdr.maxvolts) == np.float32(want_hdr.maxvolts)
    assert hdr.flags == want_hdr.flags, (hex(hdr.flags), hex(want_hdr.flags))
    got = host_rows(be, rows)
    assert got.shape == want_rows.shape and np.array_equal(got, want_rows)


def check_golden_tap(name, tmp_path, be, lib_path=None, fe_factory=None):
    """CSV text -> read_csv_device -> decode_tape takes the rows as they are -> the reference's .tap."""
    from readtape_amd import pipeline
    z, kw, _, _, dorder = golden_options(name)
    path = str(tmp_path / "c.csv")
    open(path, "wb").write(z["csv"].tobytes())
    hdr, rows, _ = csvin.read_csv_device(path, _lib_path=lib_path, _backend=be, **kw)
    tap = str(tmp_path / "c.tap")
    pipeline.decode_tape(hdr, rows, tap, fe_factory=fe_factory, trkorder=dorder)
    got, want = open(tap, "rb").read(), z["tap"].tobytes()
    assert got == want and len(want) > 40
    return rows


class Index:
    """rtfe_csv_index alone on a backend's memory."""

    def __init__(self, be, lib_path=None):
        self.be, self.lib = be, frontend._load_library(lib_path)

    def __call__(self, text, is_last, starts_cap):
        be, lib = self.be, self.lib
        dev = csvin._Dev(be, False)
        d_text = dev.alloc(len(text) + 16)
        if len(text):
            be.upload(d_text, text)
        d_starts = dev.alloc(4 * (starts_cap + 1) + 64)
        guard = np.full(16, 0xA5A5A5A5, dtype=np.uint32)
        be.upload(d_starts[4 * (starts_cap + 1):], guard.tobytes())
        scratch = dev.alloc(lib.rtfe_csv_index_scratch_bytes(len(text)))
        out = dev.alloc(32)
        rc = lib.rtfe_csv_index(be.ptr(d_text), len(text), int(is_last), be.ptr(d_starts), starts_cap, be.ptr(scratch), int(scratch.shape[0]), be.ptr(out), be.stream())
        assert rc == 0, lib.rtfe_last_error()
        be.sync()
        o = csvin._Window.from_buffer_copy(bytes(be.to_numpy(out[:24], np.uint8)))
        table = be.to_numpy(d_starts, np.uint32).copy()
        assert np.array_equal(table[starts_cap + 1: starts_cap + 17], guard), "rtfe_csv_index wrote behind starts_cap + 1 entries"
        return table[: starts_cap + 1], o


def run_index_cases(idx):
    """starts, lines, consumed and longest of rtfe_csv_index against csv_shapes.index_reference, on texts with newlines at every edge of a lane's 16 bytes
    and of a 4 KB block, a block without a newline, no newline at all, and nothing."""
    import csv_shapes
    rng = np.random.RandomState(3)
    texts = [b"", b"\n", b"a", b"a\n", b"\n\n\n", b"x" * 15 + b"\n", b"x" * 16 + b"\n" + b"y" * 14 + b"\n\n", b"x" * 4095 + b"\n\n" + b"y" * 10,
             b"ab\n" + b"z" * 5000 + b"\ncd\n" + b"q" * 9000, b"k" * 10000]
    for n in (100, 4096, 4097, 12345):
        a = rng.randint(48, 58, n).astype(np.uint8)
        a[rng.rand(n) < 0.03] = 10
        texts.append(a.tobytes())
    for text in texts:
        for is_last in (False, True):
            starts, lines, consumed, longest = csv_shapes.index_reference(text, is_last)
            table, o = idx(text, is_last, lines + 3)
            assert (o.lines, o.consumed, o.longest, o.flags) == (lines, consumed, longest, 0), (len(text), is_last, o.lines, o.consumed, o.longest, o.flags)
            assert list(table[: lines + 1]) == starts and table[lines] == consumed


def run_starts_cap_cases(idx):
    """A window with more lines than starts_cap: the flag, the entries that fit, nothing behind them (Index checks the words behind the table)."""
    import csv_shapes
    text = b"".join(b"%d\n" % i for i in range(300)) + b"tail"
    starts, lines, consumed, longest = csv_shapes.index_reference(text, True)
    for cap in (0, 1, 7, lines - 1):
        table, o = idx(text, True, cap)
        assert o.flags == csvin.CSV_STARTS_FULL and (o.lines, o.consumed, o.longest) == (lines, consumed, longest)
        assert list(table[: cap + 1]) == starts[: cap + 1]
    table, o = idx(text, True, lines)
    assert o.flags == 0 and list(table) == starts
