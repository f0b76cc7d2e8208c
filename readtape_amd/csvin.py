"""CSV ingest: a logic-analyser export ("time, v0, v1, ..." behind two title lines) -> TBIN header + int16 rows,
with the numbers the reference's converter writes (src/csvtbin.c:619-716; parser and quantiser in csrc/host/rt_csv.c).
The decode then is the .tbin decode: the reference's direct CSV path (src/readtape.c:1426-1448) works on the unquantised floats and
on the file's rounded timestamps, which no int16 front end can follow bit for bit - its author's own recommended route is the
converter ("tbin is still smaller and faster", src/readtape.c:343)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import frontend, tbin

HERE = os.path.dirname(os.path.abspath(__file__))


class _Info(C.Structure):
    _fields_ = [("columns", C.c_int), ("rows", C.c_int64), ("tstart_ns", C.c_uint64), ("tdelta_ns", C.c_uint32), ("maxvolts", C.c_float)]


def _lib():
    lib = C.CDLL(os.path.join(HERE, "librtdecode.so"))
    lib.rt_csv_survey.argtypes = [C.c_char_p, C.c_int, C.c_float, C.c_int, C.c_float, C.POINTER(_Info)]
    lib.rt_csv_load.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    lib.rt_csv_load.restype = C.c_int64
    lib.rt_csv_survey_n.argtypes = [C.c_char_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int64, C.POINTER(_Info)]
    lib.rt_csv_scan_time.argtypes = [C.c_char_p]
    lib.rt_csv_scan_time.restype = C.c_double
    lib.rt_read_mt.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int]
    return lib


def _order_flags(ntrks, mode, order, invert):
    """-> (perm or None, header flags, header trkorder) for the converter's -order= / -invert (read_csv's docstring)."""
    perm = None
    flags = tbin.FLAG_INVERTED if invert else 0
    trkorder = ""
    if order and mode == tbin.MODE_WW:
        # Whirlwind: the string goes into the header extension as it is, no column moves (src/csvtbin.c:317-323)
        if len(order) != ntrks:
            raise ValueError(f"Whirlwind -order string {order!r} does not name {ntrks} tracks")
        trkorder = order
        flags |= tbin.FLAG_NO_REORDER                  # (write_tbin adds TRKORDER_INCLUDED for a header that carries a string)
    elif order:
        h2t = frontend.parse_track_order(order)
        perm = (C.c_int * ntrks)(*h2t)
    else:
        flags |= tbin.FLAG_NO_REORDER                  # "marking the .tbin file to show it wasn't given" (src/csvtbin.c:804-807): a later -order= applies
    return perm, flags, trkorder


def read_csv(path: str, ntrks: int = 9, mode: int = tbin.MODE_NRZI, bpi: float = 0.0, ips: float = 0.0, order: str | None = None,
             invert: bool = False, scale: float = 1.0, subsample: int = 1, maxvolts: float = 0.0, descr: str = "", _preread_rows: int | None = None):
    """-> (TbinHeader, rows[n, ntrks] int16, {clipped_samples, columns}).  order = the converter's -order= string: column k of the file is that track, and
    goes to that column of the rows (src/csvtbin.c:330-352) - the file is then in track order and says so (no TBIN_NO_REORDER).  Without
    an order the header is marked TBIN_NO_REORDER (src/csvtbin.c:804-807) and a decode's trkorder= applies; a Whirlwind order string is
    kept in the header extension, columns unmoved (src/csvtbin.c:317-323).  _preread_rows: a hook for the tests - the length of the survey's
    pre-read (a million lines)."""
    lib = _lib()
    info = _Info()
    if _preread_rows is None:
        rc = lib.rt_csv_survey(path.encode(), ntrks, scale, subsample, maxvolts, C.byref(info))
    else:
        rc = lib.rt_csv_survey_n(path.encode(), ntrks, scale, subsample, maxvolts, int(_preread_rows), C.byref(info))
    if rc != 0:
        raise OSError(f"cannot read {path} as a CSV sample file ({rc})")
    perm, flags, trkorder = _order_flags(ntrks, mode, order, invert)
    rows = np.empty((max(int(info.rows), 1), ntrks), dtype=np.int16)
    clipped = C.c_int64()
    n = lib.rt_csv_load(path.encode(), ntrks, perm, int(invert), scale, subsample, info.maxvolts, rows.ctypes.data, rows.shape[0], C.byref(clipped))
    if n in (-3, -4):
        raise ValueError(f"ntrks {ntrks} or the track order is out of range for a CSV sample file")
    if n < 0:
        raise OSError(f"cannot read {path}")
    hdr = tbin.TbinHeader(ntrks=ntrks, tdelta_ns=int(info.tdelta_ns), maxvolts=float(info.maxvolts), mode=mode, bpi=bpi, ips=ips, flags=flags,
                          tstart_ns=int(info.tstart_ns), descr=descr, trkorder=trkorder)
    return hdr, rows[:n], dict(clipped_samples=int(clipped.value), columns=int(info.columns))


# ---- the same conversion on the device: the text goes to HBM once, rtfe_csv_index / _peak / _parse (include/rt_frontend.h) make the rows there ----
HOST_LINE_CHARS = 399          # what fgets(line, 400) returns whole (LINE_MAX_CHARS - 1, csrc/host/rt_csv.c): a longer line the host splits in two
PREREAD_ROWS = 1000000         # PREREAD_ROWS, csrc/host/rt_csv.c
CSV_STARTS_FULL = 1            # RTFE_CSV_STARTS_FULL


class _Window(C.Structure):
    _fields_ = [("lines", C.c_int64), ("consumed", C.c_int64), ("longest", C.c_uint32), ("flags", C.c_uint32)]


def _c_int_f32(x) -> int:
    """(int)x of a float as the host's cvttss2si gives it: INT_MIN for what does not fit."""
    x = float(x)
    return int(x) if -2147483648.0 <= x < 2147483648.0 else -2147483648


class _Dev:
    """Device memory for the text, the line starts and the rows: torch tensors on the GPU, numpy arrays under the emulator (frontend's backends)."""

    def __init__(self, be, timing):
        self.be, self.torch = be, getattr(be, "torch", None)
        self.ms = dict(upload=[], index=[], peak=[], parse=[]) if (timing and self.torch is not None) else None
        self.pin = None

    def alloc(self, nbytes):
        """nbytes of device memory from a 16-byte boundary, as a byte view."""
        buf = self.be.empty(int(nbytes) + 32)
        off = -self.be.ptr(buf) % 16
        return buf[off: off + int(nbytes) + 16]

    def zero(self, view):
        if self.torch is not None:
            view.zero_()
        else:
            view[...] = 0

    def copy(self, dst, src):
        if self.torch is not None:
            dst.copy_(src, non_blocking=True)
        else:
            dst[...] = src

    def timed(self, key):
        """A context that brackets what is queued inside it with two events on the stream (tools/gpu_csv_time.py)."""
        dev = self

        class _T:
            def __enter__(s):
                if dev.ms is not None:
                    s.e0, s.e1 = dev.torch.cuda.Event(enable_timing=True), dev.torch.cuda.Event(enable_timing=True)
                    s.e0.record()

            def __exit__(s, *a):
                if dev.ms is not None:
                    s.e1.record()
                    dev.ms[key].append((s.e0, s.e1))
        return _T()

    def read_into(self, f, dlib, pos, n, dst, cap):
        """File bytes [pos, pos + n) -> dst[:n] on the device: through one page-locked staging buffer (the upload of the window before has been waited for), read by
        rt_read_mt's threads where that pays; every byte crosses PCIe once."""
        if n <= 0:
            return
        if self.torch is None:
            f.seek(pos)
            self.be.upload(dst, f.read(n))
            return
        if self.pin is None or self.pin.numel() < n:
            self.pin = self.be.pinned(max(n, cap))
        host = self.pin.numpy()
        if n >= (8 << 20):
            if dlib.rt_read_mt(f.fileno(), host.ctypes.data, pos, n, 8) != 0:
                raise IOError("short read")
        else:
            f.seek(pos)
            if f.readinto(memoryview(host)[:n]) != n:
                raise IOError("short read")
        with self.timed("upload"):
            dst[:n].copy_(self.pin[:n], non_blocking=True)

    def total_ms(self):
        if self.ms is None:
            return None
        self.be.sync()
        return {k: float(sum(a.elapsed_time(b) for a, b in v)) for k, v in self.ms.items()}


def read_csv_device(path: str, ntrks: int = 9, mode: int = tbin.MODE_NRZI, bpi: float = 0.0, ips: float = 0.0, order: str | None = None,
                    invert: bool = False, scale: float = 1.0, subsample: int = 1, maxvolts: float = 0.0, descr: str = "",
                    window_bytes: int = 1 << 28, device="cuda:0", _lib_path=None, _backend=None, _preread_rows: int | None = None, _timing: bool = False):
    """read_csv with the conversion on the device -> (TbinHeader, rows[n, ntrks] int16 ON THE DEVICE - contiguous, 16-byte aligned, what pipeline.decode_tape and
    FrontEnd.scan take -, {clipped_samples, columns, windows, path}).  Header and rows are read_csv's, field for field and code for code.

    The file is read once, in windows of window_bytes cut on line boundaries (the bytes behind a window's last complete line are carried to the front of the
    next one, on the device), and every byte crosses PCIe once.  The survey is rt_csv_survey's: two title lines, the peak of at most a million - 1 data lines
    (rtfe_csv_peak), the period from the first and the last surveyed timestamp (the two numbers the host parses).  The windows that hold the surveyed lines stay
    resident until the full scale is known and they are parsed (rtfe_csv_parse); behind them two windows of text are resident at a time.
    A file the host would read differently - a line longer than fgets(line, 400) returns whole, a line longer than a window, a negative first timestamp - is
    handed to read_csv: path = "host", the result is the host's, uploaded.  _lib_path / _backend / _preread_rows / _timing: hooks for the tests and tools/."""
    be = _backend or frontend.TorchBackend(device)
    lib = frontend._load_library(_lib_path)
    dlib = _lib()
    dev = _Dev(be, _timing)
    perm, flags, trkorder = _order_flags(ntrks, mode, order, invert)
    P = PREREAD_ROWS if _preread_rows is None else int(_preread_rows)
    sub = max(1, int(subsample))
    W = int(window_bytes)
    if W < 16 or W >= (1 << 32):
        raise ValueError(f"window_bytes {window_bytes}: 16 .. 2^32 - 1")
    scale32, given32 = float(np.float32(scale)), np.float32(maxvolts)

    def check(rc, what):
        if rc in (-3, -4):
            raise ValueError(f"ntrks {ntrks} or the track order is out of range for a CSV sample file")
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {lib.rtfe_last_error().decode()}")

    def host_path(nwindows):
        hdr, rows, info = read_csv(path, ntrks=ntrks, mode=mode, bpi=bpi, ips=ips, order=order, invert=invert, scale=scale, subsample=subsample,
                                   maxvolts=maxvolts, descr=descr, _preread_rows=_preread_rows)
        return hdr, be.rows(rows), dict(info, windows=nwindows, path="host")

    def index(w, is_last):
        """rtfe_csv_index of window w (again with a table of the right size where the guess - a line per 8 bytes - was too small) -> its rtfe_csv_window."""
        cap = w["nbytes"] // 8 + 16
        scratch = dev.alloc(lib.rtfe_csv_index_scratch_bytes(w["nbytes"]))
        out = dev.alloc(32)
        while True:
            w["starts"] = dev.alloc(4 * (cap + 1))
            with dev.timed("index"):
                check(lib.rtfe_csv_index(be.ptr(w["text"]), w["nbytes"], int(is_last), be.ptr(w["starts"]), cap, be.ptr(scratch), int(scratch.shape[0]),
                                         be.ptr(out), be.stream()), "rtfe_csv_index")
            o = _Window.from_buffer_copy(bytes(be.to_numpy(out[:24], np.uint8)))
            if not (o.flags & CSV_STARTS_FULL):
                return o
            cap = int(o.lines)

    def line_bytes(wins, g):
        """The bytes of line g of the file (a surveyed line: its window is resident)."""
        for w in wins:
            if w["g0"] <= g < w["g0"] + w["lines"]:
                i = g - w["g0"]
                a, b = (int(x) for x in be.to_numpy(w["starts"][4 * i: 4 * i + 8], np.uint32)[:2])
                return bytes(be.to_numpy(w["text"][a: b], np.uint8)[: b - a])
        raise AssertionError(f"line {g} is in no resident window")

    state = dict(rows=None, cap=0)
    clipped = dev.alloc(16)
    dev.zero(clipped)

    def parse(w, mv, total_hint):
        """Queue rtfe_csv_parse for the data lines of window w: of every `sub` lines the last one counts, numbered over the whole file."""
        d0, d1 = max(w["g0"], 2) - 2, w["g0"] + w["lines"] - 2
        if d1 <= d0:
            return
        j0, j1 = d0 // sub, d1 // sub
        if j1 > state["cap"]:                        # (the row count of a file longer than the pre-read is an estimate until its last window: grow)
            cap = max(j1, total_hint, int(state["cap"] * 1.25) + 1024, 1)
            new = dev.alloc(cap * ntrks * 2)
            if state["rows"] is not None and j0 > 0:
                dev.copy(new[: j0 * ntrks * 2], state["rows"][: j0 * ntrks * 2])
            state["rows"], state["cap"] = new, cap
        if j1 > j0:
            first = j0 * sub + sub - 1 + 2 - w["g0"]
            with dev.timed("parse"):
                check(lib.rtfe_csv_parse(be.ptr(w["text"]), be.ptr(w["starts"]), first, sub, j1 - j0, ntrks, perm, int(invert), scale32, float(mv),
                                         be.ptr(state["rows"]) + j0 * ntrks * 2, be.ptr(clipped), be.stream()), "rtfe_csv_parse")

    peak_buf = dev.alloc(16)
    dev.zero(peak_buf)
    prefix, surveyed_all, mv = [], False, None
    tstart = tdelta = columns = 0
    nwindows, g, pos, prev = 0, 0, 0, None
    with open(path, "rb", buffering=0) as f:
        size = os.fstat(f.fileno()).st_size
        W = min(W, max(size, 16))                                    # (a short file: one window of its own length)
        while True:
            carry = 0 if prev is None else prev["nbytes"] - prev["consumed"]
            n = min(W - carry, size - pos)
            w = dict(text=dev.alloc(W), nbytes=carry + n, g0=g)
            if carry:
                dev.copy(w["text"][:carry], prev["text"][prev["consumed"]: prev["nbytes"]])
            dev.read_into(f, dlib, pos, n, w["text"][carry: carry + n], W)
            pos += n
            is_last = pos >= size
            o = index(w, is_last)
            nwindows += 1
            w["lines"], w["consumed"] = int(o.lines), int(o.consumed)
            if o.longest > HOST_LINE_CHARS or (w["lines"] == 0 and not is_last):
                return host_path(nwindows)
            g += w["lines"]
            if not surveyed_all:
                # the survey: data lines 1 .. P - 1 (the file's lines 2 .. P): their peak here, queued behind the window's index
                prefix.append(w)
                lo, hi = max(w["g0"], 2), min(g, 2 + max(P - 1, 0))
                if hi > lo:
                    with dev.timed("peak"):
                        check(lib.rtfe_csv_peak(be.ptr(w["text"]), be.ptr(w["starts"]), lo - w["g0"], hi - lo, ntrks, scale32, be.ptr(peak_buf), be.stream()), "rtfe_csv_peak")
                if g >= 2 + max(P - 1, 0) or is_last:
                    surveyed_all = True
                    if g < 2:
                        raise OSError(f"cannot read {path} as a CSV sample file (-2)")
                    title = line_bytes(prefix, 1)
                    columns = title.split(b"\0")[0].count(b",")
                    m = min(g - 2, max(P - 1, 0))                     # surveyed lines
                    if m >= 1:
                        t_first = dlib.rt_csv_scan_time(line_bytes(prefix, 2))
                        if t_first < 0:                              # (the host takes a negative time for "no first line yet" and starts over at every line)
                            return host_path(nwindows)
                        tstart = int((t_first + 0.5e-9) * 1e9)
                        if m >= 2:
                            t_last = dlib.rt_csv_scan_time(line_bytes(prefix, 2 + m - 1))
                            tdelta = int(((t_last - t_first) / float(m - 1) + 0.5e-9) * 1e9) & 0xFFFFFFFF
                    peak = be.to_numpy(peak_buf[:4], np.float32)[0]
                    with np.errstate(all="ignore"):
                        peak = np.float32(_c_int_f32((peak + np.float32(0.55)) * np.float32(10.0))) / np.float32(10.0)
                    mv = given32 if given32 > peak else peak
                    if sub > 1:
                        tstart += (sub - 1) * tdelta
                        tdelta = (tdelta * sub) & 0xFFFFFFFF
                    # the rows: known if the file ended inside the pre-read, else estimated from the bytes a line took so far
                    hint = (g - 2) // sub if is_last else int((g + (size - pos) / max(pos / max(g, 1), 1.0) * 1.02) // sub) + 1024
                    for pw in prefix:
                        parse(pw, mv, hint)
                    prefix = []
            else:
                parse(w, mv, 0)
            prev = w                                                 # (the window before it is released: two windows of text behind the pre-read)
            if is_last:
                break
    nrows = max(g - 2, 0) // sub
    nclip = int(be.to_numpy(clipped[:8], np.int64)[0])               # (synchronises: the rows are complete)
    if state["rows"] is None:
        state["rows"] = dev.alloc(max(ntrks * 2, 16))
    flat = state["rows"][: nrows * ntrks * 2]
    rows = flat.view(dev.torch.int16 if dev.torch is not None else np.int16).reshape(nrows, ntrks)
    hdr = tbin.TbinHeader(ntrks=ntrks, tdelta_ns=int(tdelta), maxvolts=float(mv), mode=mode, bpi=bpi, ips=ips, flags=flags,
                          tstart_ns=int(tstart), descr=descr, trkorder=trkorder)
    info = dict(clipped_samples=nclip, columns=int(columns), windows=nwindows, path="device")
    ms = dev.total_ms()
    if ms is not None:
        info["ms"] = ms
    return hdr, rows, info
