"""CSV export (the converter's -read, src/csvtbin.c:523-596): TBIN header + int16 rows -> the text a spreadsheet or a plot takes, byte for byte what
`csvtbin -read` prints - two title lines, then per row "%12.8f, " of the time and "%9.5f, " of every column's voltage.  csvin's other direction.

  write_csv          the host path: fprintf, csrc/host/rt_csvout.c
  write_csv_device   rows resident on the device -> text made there (rtfe_csv_format, csrc/rtfe_csvout.hip), copied out window by window
  export_window      the rows that -skip / -starttime / -endtime / -stopaft leave

Limits of the device path (rtfe_csv_format refuses what is outside; write_csv has none): |maxvolts| * 32768 / 32767 + (ntrks - 1) * |stagger| below 2^20 volts,
the last printed time below 2^49 ns (6.5 days)."""
from __future__ import annotations

import ctypes as C
import os
import queue
import threading
import time

import numpy as np

from . import csvin, frontend, tbin

HERE = os.path.dirname(os.path.abspath(__file__))
CSV_TEXT_FULL = 1              # RTFE_CSV_TEXT_FULL


class _FormatArgs(C.Structure):
    _fields_ = [("ntrks", C.c_int), ("invert", C.c_int), ("maxvolts", C.c_float), ("stagger", C.c_float), ("tstart_ns", C.c_uint64), ("tdelta_ns", C.c_uint32),
                ("perm", C.POINTER(C.c_int))]


class _Text(C.Structure):
    _fields_ = [("bytes", C.c_uint64), ("rows", C.c_int64), ("flags", C.c_uint32), ("longest", C.c_uint32)]


def _lib():
    lib = C.CDLL(os.path.join(HERE, "librtdecode.so"))
    lib.rt_csv_export_window.argtypes = [C.c_uint64, C.c_uint32, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.rt_csv_export_write.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_float, C.c_float, C.c_uint64, C.c_uint32, C.c_void_p,
                                        C.c_int64, C.c_int64]
    lib.rt_csv_export_write.restype = C.c_int64
    return lib


def title_lines(hdr: tbin.TbinHeader) -> bytes:
    """The two lines in front of the rows (src/csvtbin.c:553-555)."""
    return b"'" + hdr.descr.encode("ascii", "replace") + b"\nTime, " + b", ".join(b"Track %d" % k for k in range(hdr.ntrks)) + b"\n"


def _perm(hdr, order):
    """The converter's -order= string -> the column of the rows that field k prints (csvin._order_flags: the same string the ingest takes)."""
    return csvin._order_flags(hdr.ntrks, hdr.mode, order, False)[0]


def export_window(hdr: tbin.TbinHeader, nrows: int, skip: int = 0, starttime: float = 0.0, endtime: float = 0.0, stopaft: int | None = None):
    """-> (first, count): the rows a -read with these options prints of a tape of nrows rows (the end mark taken off).  skip rows go first, and rows
    before starttime seconds (with either option at least one row goes: the reference's loop is a do-while); then rows are printed until stopaft of them
    are, or one has been printed whose successor's time lies behind endtime.  0 / None: not given."""
    first, count = C.c_int64(), C.c_int64()
    rc = _lib().rt_csv_export_window(int(hdr.tstart_ns), int(hdr.tdelta_ns), int(nrows), int(skip), float(starttime), float(endtime), int(stopaft or 0),
                                     C.byref(first), C.byref(count))
    if rc != 0:
        raise ValueError(f"export_window: bad arguments ({rc})")
    return int(first.value), int(count.value)


def write_csv(path: str, hdr: tbin.TbinHeader, rows, order: str | None = None, stagger: float = 0.0, **window):
    """rows[n, ntrks] int16 (host) -> the file `csvtbin -read` writes for the .tbin of (hdr, rows): the rows end at the first -32768 in column 0, the tape
    is inverted if the header says so (TBIN_INVERTED), order / stagger / **window (export_window's options) are the converter's -order= / -stagger= /
    -skip= ... .  -> dict(rows=, bytes=)."""
    rows = np.ascontiguousarray(rows, dtype=np.int16)
    assert rows.ndim == 2 and rows.shape[1] == hdr.ntrks
    ends = np.flatnonzero(rows[:, 0] == tbin.END_MARK)
    n = int(ends[0]) if ends.size else rows.shape[0]
    first, count = export_window(hdr, n, **window)
    nbytes = _lib().rt_csv_export_write(path.encode(), hdr.descr.encode("ascii", "replace"), hdr.ntrks, _perm(hdr, order), int(bool(hdr.flags & tbin.FLAG_INVERTED)),
                                        float(hdr.maxvolts), float(stagger), int(hdr.tstart_ns), int(hdr.tdelta_ns), rows.ctypes.data, first, count)
    if nbytes in (-3, -4):
        raise ValueError(f"ntrks {hdr.ntrks} or the track order is out of range for a CSV sample file")
    if nbytes < 0:
        raise OSError(f"cannot write {path} ({nbytes})")
    return dict(rows=count, bytes=int(nbytes))


def format_args(hdr: tbin.TbinHeader, order: str | None = None, stagger: float = 0.0) -> _FormatArgs:
    """rtfe_csv_format's arguments for a tape (the perm array stays alive with the structure)."""
    perm = _perm(hdr, order)
    a = _FormatArgs(hdr.ntrks, int(bool(hdr.flags & tbin.FLAG_INVERTED)), float(hdr.maxvolts), float(stagger), int(hdr.tstart_ns), int(hdr.tdelta_ns),
                    C.cast(perm, C.POINTER(C.c_int)) if perm is not None else None)
    a._perm = perm
    return a


def _find_end(lib, be, lib_path, d_rows, nrows, ntrks):
    """The first row whose column 0 holds the end mark, or nrows: rtfe_find_end_mark.  It wants a handle (for the track count and the chip's size): one
    that any header gives - the tape's own parameters play no part in the search."""
    if nrows == 0:
        return 0
    cfg = frontend.FrontEndConfig(mode=frontend.NRZI, ntrks=ntrks, maxvolts=1.0, bpi=0.0, ips=50.0, tdelta_ns=1000, parmsets=frontend.DEFAULT_PARMSETS[frontend.NRZI][:1])
    fe = frontend.FrontEnd(cfg, _lib_path=lib_path, _backend=be)
    try:
        first = be.empty(16)
        if lib.rtfe_find_end_mark(fe.h, be.ptr(d_rows), nrows, be.ptr(first), be.stream()) != 0:
            raise RuntimeError(f"rtfe_find_end_mark failed: {lib.rtfe_last_error().decode()}")
        f = int(be.to_numpy(first[:8], np.int64)[0])
    finally:
        fe.close()
    return min(f, nrows)


def write_csv_device(path: str, hdr: tbin.TbinHeader, rows, order: str | None = None, stagger: float = 0.0, window_rows: int = 1 << 22, _lib_path=None,
                     _backend=None, **window):
    """write_csv with the text made on the device.  rows: an int16 [n, ntrks] device tensor, contiguous (what read_csv_device returns and decode_tape
    takes), or a numpy array (uploaded; the emulator's backend takes only that).  The file is write_csv's, byte for byte.

    The end mark is found on the device (rtfe_find_end_mark), the window options are applied (export_window), and the rows that remain go through
    rtfe_csv_format window_rows at a time: window k is formatted into one of two device buffers while window k - 1 is copied to page-locked memory on a
    copy stream and a writer thread puts window k - 2 into the file.  A window whose lines provably all have 14 + 11 ntrks + 1 bytes takes the uniform
    path (a line's place is a multiplication), any other the general one (a length pass and a prefix sum first): path = "uniform" | "general" | "mixed".
    -> dict(rows=, bytes=, path=, windows=, ms=dict(format= the kernels by stream events (None under the emulator), total= wall clock))."""
    t_enter = time.perf_counter()
    be = _backend or frontend.TorchBackend()
    torch = getattr(be, "torch", None)
    lib = frontend._load_library(_lib_path)
    ntrks = hdr.ntrks
    if not 1 <= ntrks <= 19:
        raise ValueError(f"ntrks {ntrks} is out of range for a CSV sample file")
    args = format_args(hdr, order, stagger)
    W = int(window_rows)
    if W < 1:
        raise ValueError(f"window_rows {window_rows}: at least 1")
    d_rows = be.rows(rows)
    if d_rows.ndim != 2 or d_rows.shape[1] != ntrks:
        raise ValueError(f"rows of shape {tuple(d_rows.shape)} for a tape of {ntrks} tracks")
    n = _find_end(lib, be, _lib_path, d_rows, int(d_rows.shape[0]), ntrks)
    first, count = export_window(hdr, n, **window)

    def check(rc, what):
        if rc in (-3, -4):
            raise ValueError(f"ntrks {ntrks} or the track order is out of range for a CSV sample file")
        if rc < 0:
            raise ValueError(f"{what} refused ({rc}): {lib.rtfe_last_error().decode()}")
        return rc

    spans = [(r, min(W, first + count - r)) for r in range(first, first + count, W)]
    uniform = [check(lib.rtfe_csv_format_path(r, m, C.byref(args)), "rtfe_csv_format_path") == 1 for r, m in spans]      # (every refusal comes before the file is touched)
    line = 14 + 11 * ntrks + 1
    caps = [m * line if u else int(lib.rtfe_csv_format_max_bytes(m, ntrks)) for (r, m), u in zip(spans, uniform)]
    dev = csvin._Dev(be, False)
    cap = max(caps, default=0)
    text = [dev.alloc(cap + 16) for _ in range(min(2, len(spans)))]
    outs = [dev.alloc(32) for _ in text]
    scratch = [dev.alloc(lib.rtfe_csv_format_scratch_bytes(min(W, max(count, 1)))) for _ in text]
    events, total = [], 0

    def launch(k):
        r, m = spans[k]
        b = k % 2
        if torch is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        check(lib.rtfe_csv_format(be.ptr(d_rows), r, m, C.byref(args), be.ptr(text[b]), caps[k], be.ptr(scratch[b]), int(scratch[b].shape[0]), be.ptr(outs[b]),
                                  be.stream()), "rtfe_csv_format")
        if torch is not None:
            e1.record()
            events.append((e0, e1))
            return e1

    def result(k):
        o = _Text.from_buffer_copy(bytes(be.to_numpy(outs[k % 2][:24], np.uint8)))      # (synchronises with window k's kernels)
        if o.flags & CSV_TEXT_FULL or o.rows != spans[k][1] or (uniform[k] and o.bytes != caps[k]):
            raise RuntimeError(f"rtfe_csv_format: window {k} reports {o.bytes} bytes for a buffer of {caps[k]}")
        return int(o.bytes)

    with open(path, "wb", buffering=0) as f:
        f.write(title_lines(hdr))
        total += len(title_lines(hdr))
        if torch is None:
            for k in range(len(spans)):
                launch(k)
                nb = result(k)
                f.write(text[k % 2][:nb].tobytes())
                total += nb
        elif spans:
            copy_stream = torch.cuda.Stream(be.device)
            pins = [be.pinned(cap) for _ in text]
            jobs, errors = queue.Queue(), []
            written = [threading.Event() for _ in spans]

            def writer():
                while True:
                    job = jobs.get()
                    if job is None:
                        return
                    k, nb = job
                    try:
                        if not errors:
                            mv, done = memoryview(pins[k % 2].numpy())[:nb], 0
                            while done < nb:
                                done += f.write(mv[done:])
                    except Exception as e:                      # (kept for the caller's thread; the windows behind it are let through unwritten)
                        errors.append(e)
                    written[k].set()
            th = threading.Thread(target=writer, daemon=True)
            th.start()
            try:
                done_fmt = launch(0)
                for k in range(len(spans)):
                    nb = result(k)
                    total += nb
                    if k >= 2:
                        written[k - 2].wait()                  # its pinned buffer is free again
                    with torch.cuda.stream(copy_stream):
                        copy_stream.wait_event(done_fmt)
                        pins[k % 2][:nb].copy_(text[k % 2][:nb], non_blocking=True)
                        copied = torch.cuda.Event()
                        copied.record(copy_stream)
                    if k + 1 < len(spans):
                        done_fmt = launch(k + 1)               # (the other device buffer: window k - 1's copy out of it was waited for below)
                    copied.synchronize()
                    jobs.put((k, nb))
            finally:
                jobs.put(None)
                th.join()
            if errors:
                raise errors[0]
    ms = dict(format=None, total=(time.perf_counter() - t_enter) * 1e3)
    if torch is not None:
        be.sync()
        ms["format"] = float(sum(a.elapsed_time(b) for a, b in events))
    kinds = set(uniform)
    return dict(rows=count, bytes=total, path="mixed" if len(kinds) > 1 else ("general" if kinds == {False} else "uniform"), windows=len(spans), ms=ms)
