"""CSV ingest: a logic-analyser export ("time, v0, v1, ..." behind two title lines) -> TBIN header + int16 rows,
with the numbers the reference's converter writes (src/csvtbin.c:619-716; parser and quantiser in csrc/host/rt_csv.c).
The decode then is the .tbin decode: the reference's direct CSV path (src/readtape.c:1426-1448) works on the unquantised floats and
on the file's rounded timestamps, which no int16 front end can follow bit for bit - its author's own recommended route is the
converter ("tbin is still smaller and faster", src/readtape.c:343)."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import queue
import threading

import numpy as np

from . import frontend, tbin

HERE = os.path.dirname(os.path.abspath(__file__))


class _Info(C.Structure):
    _fields_ = [("columns", C.c_int), ("rows", C.c_int64), ("tstart_ns", C.c_uint64), ("tdelta_ns", C.c_uint32), ("maxvolts", C.c_float)]


class _ConvWindow(C.Structure):
    _fields_ = [("skipped", C.c_int64), ("first_line", C.c_int64), ("count", C.c_int64), ("ended", C.c_int)]


class _PassOpts(C.Structure):
    _fields_ = [("ntrks", C.c_int), ("perm", C.POINTER(C.c_int)), ("invert", C.c_int), ("scale", C.c_float), ("subsample", C.c_int), ("maxvolts", C.c_float),
                ("skip", C.c_int64), ("starttime", C.c_float), ("endtime", C.c_float), ("stopaft", C.c_int64), ("graphbin", C.c_int64),
                ("tstart_ns", C.c_uint64), ("tdelta_ns", C.c_uint32)]


class _Pass(C.Structure):
    _fields_ = [("skipped", C.c_int64), ("samples", C.c_int64), ("too_big", C.c_int64), ("too_small", C.c_int64), ("graph_lines", C.c_int64),
                ("ended", C.c_int), ("newmax", C.c_float)]


ENDED = ("file", "stopaft", "endtime")          # RT_CSV_ENDED_*


def _lib():
    lib = C.CDLL(os.path.join(HERE, "librtdecode.so"))
    lib.rt_csv_convert_window.argtypes = [C.c_uint64, C.c_uint32, C.c_int64, C.c_int, C.c_int64, C.c_float, C.c_float, C.c_int64, C.POINTER(_ConvWindow)]
    lib.rt_csv_redo_maxvolts.argtypes = [C.c_float]
    lib.rt_csv_redo_maxvolts.restype = C.c_float
    lib.rt_csv_convert_pass.argtypes = [C.c_char_p, C.POINTER(_PassOpts), C.c_void_p, C.c_int64, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_void_p, C.c_void_p,
                                        C.c_int64, C.POINTER(_Pass)]
    lib.rt_csv_graph_write.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_int64]
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


def _window_options(skip, starttime, endtime, stopaft, graph, subsample=1):
    """The converter's -skip= / -starttime= / -endtime= / -stopaft= / -graph= as its option parser takes them (src/csvtbin.c:364-376, 397), refused
    where it refuses them -> (skip, starttime, endtime, stopaft, graph), 0 standing for "not given".  (A subsample below 1 is taken as 1, as the loader
    has always taken it.)"""
    skip, graph, stopaft = int(skip or 0), int(graph or 0), (None if stopaft is None else int(stopaft))
    starttime, endtime = float(np.float32(starttime or 0.0)), float(np.float32(endtime or 0.0))
    if skip < 0 or skip >= (1 << 63):
        raise ValueError(f"skip {skip}: 0 or more lines")
    if stopaft is not None and not 1 <= stopaft < (1 << 63):
        raise ValueError(f"stopaft {stopaft}: at least 1 sample")
    for name, x in (("starttime", starttime), ("endtime", endtime)):
        if x != 0.0 and not (np.float32(0.01) <= np.float32(x) <= np.float32(1000.0)):
            raise ValueError(f"{name} {x}: 0.01 .. 1000 seconds")
    if starttime and endtime and not int(float(starttime) * 1e9) < int(float(endtime) * 1e9):
        raise ValueError(f"starttime {starttime} is not before endtime {endtime}")
    if not 0 <= graph <= 0x7FFFFFFF:
        raise ValueError(f"graph {graph}: samples per bin, 1 .. 2^31 - 1")
    return skip, starttime, endtime, stopaft or 0, graph


def convert_window(tstart_ns: int, tdelta_ns: int, data_lines: int, subsample: int = 1, skip: int = 0, starttime: float = 0.0, endtime: float = 0.0,
                   stopaft: int | None = None):
    """-> dict(skipped, first_line, count, ended): the samples a conversion with these options writes of a file of data_lines raw data lines (the lines
    behind the two titles), csvout.export_window's counterpart.  tstart_ns / tdelta_ns: the header's, after the -subsample adjustment.  With -skip or
    -starttime K = max(1, skip, ceil((starttime - tstart) / tdelta)) RAW lines go first (the header's tstart does not move); sample j is raw data line
    first_line + j * subsample; a sample is written, then the pass ends if stopaft samples are written or the clock tstart + (K + samples) * tdelta is
    behind endtime: ended = "stopaft" | "endtime" | "file".  A file that ends inside the skip: ValueError."""
    skip, starttime, endtime, stopaft, _ = _window_options(skip, starttime, endtime, stopaft, 0, subsample)
    w = _ConvWindow()
    rc = _lib().rt_csv_convert_window(int(tstart_ns), int(tdelta_ns), int(data_lines), max(1, int(subsample)), skip, starttime, endtime, stopaft, C.byref(w))
    if rc != 0:
        raise ValueError("the file ends with samples left to skip" if rc == -5 else f"convert_window: bad arguments ({rc})")
    return dict(skipped=int(w.skipped), first_line=int(w.first_line), count=int(w.count), ended=ENDED[w.ended])


def graph_lines(samples: int, ended: str, graph: int) -> int:
    """Lines of the graph file: a full bin per `graph` samples, but the sample on which -stopaft or -endtime ends the pass closes none."""
    if graph < 1 or samples < 1:
        return 0
    return (samples if ended == "file" else samples - 1) // graph


def _survey(lib, path, ntrks, scale, subsample, maxvolts, _preread_rows):
    info = _Info()
    if _preread_rows is None:
        rc = lib.rt_csv_survey(path.encode(), ntrks, scale, subsample, maxvolts, C.byref(info))
    else:
        rc = lib.rt_csv_survey_n(path.encode(), ntrks, scale, subsample, maxvolts, int(_preread_rows), C.byref(info))
    if rc != 0:
        raise OSError(f"cannot read {path} as a CSV sample file ({rc})")
    return info


def _host_convert(path, ntrks, mode, bpi, ips, order, invert, scale, subsample, maxvolts, descr, _preread_rows, skip, starttime, endtime, stopaft, graph, redo,
                  keep_rows, tbin_path, graph_path, times):
    """The conversion on the host, at most two passes (rt_csv_convert_pass) -> (TbinHeader, rows or None, info)."""
    lib = _lib()
    skip, starttime, endtime, stopaft, graph = _window_options(skip, starttime, endtime, stopaft, graph, subsample)
    info = _survey(lib, path, ntrks, scale, subsample, maxvolts, _preread_rows)
    perm, flags, trkorder = _order_flags(ntrks, mode, order, invert)
    if not 1 <= ntrks <= 19:
        raise ValueError(f"ntrks {ntrks} or the track order is out of range for a CSV sample file")
    cap = max(int(info.rows), 1)
    if stopaft:
        cap = min(cap, stopaft)
    rows = np.empty((cap, ntrks), dtype=np.int16) if keep_rows else None
    gcap = cap // graph + 1 if graph else 0
    g_at, g_max = np.zeros(gcap, dtype=np.int64), np.zeros(gcap, dtype=np.float32)
    mv, redone, first = float(info.maxvolts), False, None
    kw = dict(times=tuple(times)) if times is not None else {}
    for attempt in range(2):
        hdr = tbin.TbinHeader(ntrks=ntrks, tdelta_ns=int(info.tdelta_ns), maxvolts=mv, mode=mode, bpi=bpi, ips=ips, flags=flags,
                              tstart_ns=int(info.tstart_ns), descr=descr, trkorder=trkorder, **kw)
        head = tbin.pack_header(hdr)
        o = _PassOpts(ntrks, C.cast(perm, C.POINTER(C.c_int)) if perm is not None else None, int(invert), scale, max(1, int(subsample)), mv,
                      skip if attempt == 0 else 0,             # (the first pass counted -skip down to nothing: the second skips by -starttime alone, src/csvtbin.c:678)
                      starttime, endtime, stopaft, graph if attempt == 0 else 0, int(info.tstart_ns), int(info.tdelta_ns))
        res = _Pass()
        rc = lib.rt_csv_convert_pass(path.encode(), C.byref(o), rows.ctypes.data if keep_rows else None, cap, tbin_path.encode() if tbin_path else None, head, len(head),
                                     graph_path.encode() if (graph_path and graph and attempt == 0) else None, g_at.ctypes.data, g_max.ctypes.data, gcap, C.byref(res))
        if rc in (-3, -4):
            raise ValueError(f"ntrks {ntrks} or the track order is out of range for a CSV sample file")
        if rc == -5:
            raise ValueError(f"{path} ends with samples left to skip")
        if rc != 0:
            raise OSError(f"cannot convert {path} ({rc})")
        if attempt == 0:
            first = res
            ngraph = int(res.graph_lines)
        if not (redo and attempt == 0 and (res.too_big or res.too_small)):
            break
        mv, redone = float(lib.rt_csv_redo_maxvolts(res.newmax)), True
    out = dict(clipped_samples=int(res.too_big + res.too_small), columns=int(info.columns), skipped=int(first.skipped), samples=int(res.samples),
               too_big=int(res.too_big), too_small=int(res.too_small), redone=redone, ended=ENDED[res.ended])
    if graph:
        out["graph"] = (g_at[:ngraph].copy(), g_max[:ngraph].copy())
    return hdr, (rows[: int(res.samples)] if keep_rows else None), out


def read_csv(path: str, ntrks: int = 9, mode: int = tbin.MODE_NRZI, bpi: float = 0.0, ips: float = 0.0, order: str | None = None,
             invert: bool = False, scale: float = 1.0, subsample: int = 1, maxvolts: float = 0.0, descr: str = "", _preread_rows: int | None = None,
             skip: int = 0, starttime: float = 0.0, endtime: float = 0.0, stopaft: int | None = None, graph: int = 0, redo: bool = False):
    """-> (TbinHeader, rows[n, ntrks] int16, info).  order = the converter's -order= string: column k of the file is that track, and
    goes to that column of the rows (src/csvtbin.c:330-352) - the file is then in track order and says so (no TBIN_NO_REORDER).  Without
    an order the header is marked TBIN_NO_REORDER (src/csvtbin.c:804-807) and a decode's trkorder= applies; a Whirlwind order string is
    kept in the header extension, columns unmoved (src/csvtbin.c:317-323).  _preread_rows: a hook for the tests - the length of the survey's
    pre-read (a million lines).

    skip / starttime / endtime / stopaft: the converter's window options (convert_window states the rule; the header's tstart stays the file's).
    graph = n: info["graph"] = (sample numbers int64, float32 maxima) - per n samples the largest |volts| over all tracks, the lines of the converter's
    <base>.graph.csv.  redo: a pass that clips (a code of +-32767) is run again with the full scale sized by the largest sample of the first pass;
    the second pass skips by starttime alone (the reference has counted -skip down by then) and makes no graph.
    info: clipped_samples, columns, skipped (raw lines of the first pass), samples, too_big, too_small, redone, ended ("file" | "stopaft" | "endtime")."""
    return _host_convert(path, ntrks, mode, bpi, ips, order, invert, scale, subsample, maxvolts, descr, _preread_rows, skip, starttime, endtime, stopaft, graph, redo,
                         True, None, None, None)


def convert_csv(csv_path: str, tbin_path: str, graph_path: str | None = None, times=None, ntrks: int = 9, mode: int = tbin.MODE_NRZI, bpi: float = 0.0,
                ips: float = 0.0, order: str | None = None, invert: bool = False, scale: float = 1.0, subsample: int = 1, maxvolts: float = 0.0, descr: str = "",
                skip: int = 0, starttime: float = 0.0, endtime: float = 0.0, stopaft: int | None = None, graph: int = 0, redo: bool = False,
                _preread_rows: int | None = None):
    """File to file, what `csvtbin <options> base` makes of base.csv: tbin_path = tbin.pack_header + the rows + the end mark, and with graph = n
    graph_path (default: tbin_path's base + ".graph.csv") = a line "<sample number>, <%f of the maximum>" per n samples.  Nothing of the file is kept
    in memory.  times: the header's 27 date words (written, read, converted; the reference puts the wall clock into the third) - zeros if not given.
    -> (TbinHeader, info) with read_csv's info (the graph arrays included)."""
    if graph and graph_path is None:
        graph_path = (tbin_path[:-5] if tbin_path.endswith(".tbin") else tbin_path) + ".graph.csv"
    hdr, _, info = _host_convert(csv_path, ntrks, mode, bpi, ips, order, invert, scale, subsample, maxvolts, descr, _preread_rows, skip, starttime, endtime, stopaft,
                                 graph, redo, False, tbin_path, graph_path, times)
    return hdr, info


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
        self.ms = dict(upload=[], index=[], peak=[], parse=[], graph=[]) if (timing and self.torch is not None) else None
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


class _ResidentSink:
    """Where a pass's rows go - read_csv_device: one buffer on the device that grows (the row count of a file longer than the pre-read is an estimate until
    its last window)."""

    def __init__(self, dev, ntrks):
        self.dev, self.ntrks, self.rows, self.cap = dev, ntrks, None, 0

    def start(self, hdr):
        pass

    def window(self, j0, nk, total_hint):
        """-> the address for rows j0 .. j0 + nk of the pass."""
        dev, rb = self.dev, self.ntrks * 2
        if j0 + nk > self.cap:
            cap = max(j0 + nk, total_hint, int(self.cap * 1.25) + 1024, 1)
            new = dev.alloc(cap * rb)
            if self.rows is not None and j0 > 0:
                dev.copy(new[: j0 * rb], self.rows[: j0 * rb])
            self.rows, self.cap = new, cap
        return dev.be.ptr(self.rows) + j0 * rb

    def queued(self, nk):
        pass

    def finish(self, nrows, clipped):
        """-> (rows[nrows, ntrks] on the device, the codes at the upper rail - looked for only where something clipped)."""
        dev = self.dev
        if self.rows is None:
            self.rows = dev.alloc(max(self.ntrks * 2, 16))
        flat = self.rows[: nrows * self.ntrks * 2]
        rows = flat.view(dev.torch.int16 if dev.torch is not None else np.int16).reshape(nrows, self.ntrks)
        return rows, (int((rows == 32767).sum()) if clipped else 0)

    def abort(self):
        self.rows = None


class _FileSink:
    """Where a pass's rows go - convert_csv_device: window k's rows are made in one of two device buffers, copied to one of two page-locked buffers on a copy
    stream, and put into the .tbin by a writer thread (write_csv_device's ring, the other way round).  Under the emulator they are written as they come."""

    def __init__(self, dev, ntrks, path, times):
        self.dev, self.ntrks, self.path, self.times = dev, ntrks, path, times
        self.f, self.k, self.big = None, 0, 0
        self.bufs, self.pins, self.copied, self.written = [None, None], [None, None], {}, {}
        self.jobs, self.errors, self.th, self.copy_stream = None, [], None, None

    def start(self, hdr):
        self.f = open(self.path, "wb", buffering=0)
        self.f.write(tbin.pack_header(dataclasses.replace(hdr, times=tuple(self.times)) if self.times is not None else hdr))
        if self.dev.torch is not None:
            self.copy_stream = self.dev.torch.cuda.Stream(self.dev.be.device)
            self.jobs = queue.Queue()
            self.th = threading.Thread(target=self._writer, daemon=True)
            self.th.start()

    def _writer(self):
        while True:
            job = self.jobs.get()
            if job is None:
                return
            k, nb, copied, written = job
            try:
                if not self.errors:
                    copied.synchronize()
                    host = self.pins[k % 2].numpy()[:nb]
                    self.big += int(np.count_nonzero(host.view(np.int16) == 32767))
                    mv, done = memoryview(host), 0
                    while done < nb:
                        done += self.f.write(mv[done:])
            except Exception as e:                              # (kept for the caller's thread; the windows behind it are let through unwritten)
                self.errors.append(e)
            finally:
                written.set()

    def _wait_written(self, ev):
        while not ev.wait(1.0):
            if self.th is None or not self.th.is_alive():
                raise RuntimeError("the .tbin writer thread has ended with windows left to write")

    def window(self, j0, nk, total_hint):
        b, nb = self.k % 2, nk * self.ntrks * 2
        if self.k >= 2 and self.dev.torch is not None:
            self.copied.pop(self.k - 2).synchronize()           # the copy out of this device buffer, two windows ago
        if self.bufs[b] is None or self.bufs[b].shape[0] < nb + 16:
            self.bufs[b] = self.dev.alloc(nb)
        return self.dev.be.ptr(self.bufs[b])

    def queued(self, nk):
        k, b, nb = self.k, self.k % 2, nk * self.ntrks * 2
        self.k += 1
        torch = self.dev.torch
        if torch is None:
            host = np.asarray(self.bufs[b][:nb])
            self.big += int(np.count_nonzero(host.view(np.int16) == 32767))
            self.f.write(host.tobytes())
            return
        parsed = torch.cuda.Event()
        parsed.record()
        if k >= 2:
            self._wait_written(self.written.pop(k - 2))         # its page-locked buffer is free again
        if self.pins[b] is None or self.pins[b].numel() < nb:
            self.pins[b] = self.dev.be.pinned(nb)
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(parsed)
            self.pins[b][:nb].copy_(self.bufs[b][:nb], non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(self.copy_stream)
        self.copied[k], self.written[k] = copied, threading.Event()
        self.jobs.put((k, nb, copied, self.written[k]))         # (the writer gets the objects themselves: this thread takes them out of the tables two windows on)

    def _join(self):
        if self.th is not None:
            self.jobs.put(None)
            self.th.join()
            self.th = None

    def finish(self, nrows, clipped):
        self._join()
        try:
            if self.errors:
                raise self.errors[0]
            self.f.write(b"\x00\x80")                             # the end mark
        finally:
            self.f.close()
        return None, self.big

    def abort(self):
        self._join()
        if self.f is not None:
            self.f.close()


class _HostFile(Exception):
    """Raised inside a device pass by a file the host would read differently; carries the windows read so far."""


def _device_convert(path, make_sink, host_path, ntrks, mode, bpi, ips, order, invert, scale, subsample, maxvolts, descr, window_bytes, device, _lib_path, _backend,
                    _preread_rows, _timing, skip, starttime, endtime, stopaft, graph, redo):
    """The conversion on the device, at most two passes over the file -> (TbinHeader, what the sink's finish returns, info), or host_path()'s result for a file
    the host would read differently.  read_csv_device's docstring describes a pass."""
    skip, starttime, endtime, stopaft, graph = _window_options(skip, starttime, endtime, stopaft, graph, subsample)
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

    def window_rule(tstart, tdelta, data_lines, skip_p):
        w = _ConvWindow()
        rc = dlib.rt_csv_convert_window(int(tstart), int(tdelta), int(data_lines), sub, skip_p, starttime, endtime, stopaft, C.byref(w))
        if rc != 0:
            raise ValueError(f"{path} ends with samples left to skip")
        return w

    def survey_result(prefix, g, peak_buf, nwindows):
        """What rt_csv_survey makes of the surveyed lines, all resident in the windows `prefix` (g lines of the file seen so far, their peak in peak_buf)
        -> (tstart, tdelta, columns, full scale), the two times after the -subsample adjustment."""
        if g < 2:
            raise OSError(f"cannot read {path} as a CSV sample file (-2)")
        tstart = tdelta = 0
        columns = line_bytes(prefix, 1).split(b"\0")[0].count(b",")
        m = min(g - 2, max(P - 1, 0))                     # surveyed lines
        if m >= 1:
            t_first = dlib.rt_csv_scan_time(line_bytes(prefix, 2))
            if t_first < 0:                              # (the host takes a negative time for "no first line yet" and starts over at every line)
                raise _HostFile(nwindows)
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
        return tstart, tdelta, columns, mv

    def run_pass(known, skip_p, graph_p, want_peak):
        """One pass over the file.  known = (tstart, tdelta, columns, full scale) of an earlier pass's survey, or None: the survey is part of this pass.
        -> a dict of what the pass found; _HostFile for a file that is the host's."""
        sink = make_sink(dev)
        clipped = dev.alloc(16)
        dev.zero(clipped)
        peak_buf, pass_peak = dev.alloc(16), dev.alloc(16)
        dev.zero(peak_buf)
        dev.zero(pass_peak)
        st = dict(bins=None, nbins=0, done=0, K=0, L=0, hdr=None)

        def bins_for(nb):
            """The graph's bins, grown to nb of them (new ones zero)."""
            if nb > st["nbins"]:
                cap = max(nb, int(st["nbins"] * 1.5) + 1024)
                new = dev.alloc(4 * cap)
                dev.zero(new)
                if st["bins"] is not None:
                    dev.copy(new[: 4 * st["nbins"]], st["bins"][: 4 * st["nbins"]])
                st["bins"], st["nbins"] = new, cap
            return be.ptr(st["bins"])

        def begin(tstart, tdelta, mv):
            """The survey is done: the header, and what the window options leave (K raw lines skipped, at most L samples)."""
            st["hdr"] = tbin.TbinHeader(ntrks=ntrks, tdelta_ns=int(tdelta), maxvolts=float(mv), mode=mode, bpi=bpi, ips=ips, flags=flags,
                                        tstart_ns=int(tstart), descr=descr, trkorder=trkorder)
            w = window_rule(tstart, tdelta, 1 << 62, skip_p)
            st["K"], st["L"] = int(w.skipped), int(w.count)
            sink.start(st["hdr"])

        def parse(w, mv, total_hint):
            """Queue rtfe_csv_parse (and rtfe_csv_graph) for the samples in window w: sample j of the pass is raw data line K + j * sub + sub - 1."""
            d0, d1 = max(w["g0"], 2) - 2, w["g0"] + w["lines"] - 2
            K, L = st["K"], st["L"]
            j0, j1 = max(0, (d0 - K) // sub), min(max(0, (d1 - K) // sub), L)
            if d1 <= d0 or j1 <= j0:
                return
            first, nk = K + j0 * sub + sub - 1 + 2 - w["g0"], j1 - j0
            rows_ptr = sink.window(j0, nk, min(total_hint, L))
            with dev.timed("parse"):
                check(lib.rtfe_csv_parse(be.ptr(w["text"]), be.ptr(w["starts"]), first, sub, nk, ntrks, perm, int(invert), scale32, float(mv),
                                         rows_ptr, be.ptr(clipped), be.stream()), "rtfe_csv_parse")
            if graph_p or want_peak:
                nb = (j1 - 1) // graph_p + 1 if graph_p else 0
                with dev.timed("graph"):
                    check(lib.rtfe_csv_graph(be.ptr(w["text"]), be.ptr(w["starts"]), first, sub, nk, ntrks, scale32, j0, graph_p or 1,
                                             bins_for(nb) if nb else None, nb, be.ptr(pass_peak) if want_peak else None, be.stream()), "rtfe_csv_graph")
            sink.queued(nk)
            st["done"] = j1

        prefix, surveyed_all, mv = [], known is not None, None
        tstart = tdelta = columns = 0
        if known is not None:
            tstart, tdelta, columns, mv = known
            begin(tstart, tdelta, mv)
        nwindows, g, pos, prev = 0, 0, 0, None
        try:
            with open(path, "rb", buffering=0) as f:
                size = os.fstat(f.fileno()).st_size
                Wp = min(W, max(size, 16))                                   # (a short file: one window of its own length)
                while True:
                    carry = 0 if prev is None else prev["nbytes"] - prev["consumed"]
                    n = min(Wp - carry, size - pos)
                    w = dict(text=dev.alloc(Wp), nbytes=carry + n, g0=g)
                    if carry:
                        dev.copy(w["text"][:carry], prev["text"][prev["consumed"]: prev["nbytes"]])
                    dev.read_into(f, dlib, pos, n, w["text"][carry: carry + n], Wp)
                    pos += n
                    is_last = pos >= size
                    o = index(w, is_last)
                    nwindows += 1
                    w["lines"], w["consumed"] = int(o.lines), int(o.consumed)
                    if o.longest > HOST_LINE_CHARS or (w["lines"] == 0 and not is_last):
                        raise _HostFile(nwindows)
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
                            tstart, tdelta, columns, mv = survey_result(prefix, g, peak_buf, nwindows)
                            begin(tstart, tdelta, mv)
                            # the rows: known if the file ended inside the pre-read, else estimated from the bytes a line took so far
                            hint = (g - 2) // sub if is_last else int((g + (size - pos) / max(pos / max(g, 1), 1.0) * 1.02) // sub) + 1024
                            for pw in prefix:
                                parse(pw, mv, hint)
                            prefix = []
                    else:
                        parse(w, mv, 0)
                    prev = w                                                 # (the window before it is released: two windows of text behind the pre-read)
                    if is_last or (surveyed_all and st["done"] >= st["L"]):   # (-stopaft / -endtime have ended the pass: the rest of the file is not read)
                        break
            data_lines = max(g - 2, 0)
            rule = window_rule(tstart, tdelta, data_lines, skip_p)             # (raises for a file that ends inside the skip)
            assert rule.count == st["done"] and rule.skipped == st["K"], (rule.count, st["done"])
            nclip = int(be.to_numpy(clipped[:8], np.int64)[0])               # (synchronises: the rows are complete)
            out, big = sink.finish(int(rule.count), nclip)
        except BaseException:
            sink.abort()
            raise
        res = dict(hdr=st["hdr"], out=out, clipped=nclip, too_big=int(big), columns=int(columns), windows=nwindows, skipped=int(rule.skipped), samples=int(rule.count),
                   ended=ENDED[rule.ended], known=(tstart, tdelta, columns), peak=float(be.to_numpy(pass_peak[:4], np.float32)[0]) if want_peak else 0.0)
        if graph_p:
            ng = graph_lines(res["samples"], res["ended"], graph_p)
            mx = np.array(be.to_numpy(st["bins"][: 4 * ng], np.float32)[:ng], dtype=np.float32) if ng else np.zeros(0, dtype=np.float32)
            res["graph"] = ((np.arange(ng, dtype=np.int64) + 1) * graph_p, mx)
        return res

    try:
        last, redone = run_pass(None, skip, graph, bool(redo)), False
        first = last
        if redo and first["clipped"]:
            mv2 = float(dlib.rt_csv_redo_maxvolts(first["peak"]))
            first["out"] = None                                              # (the first pass's rows are released before the second's are made)
            last, redone = run_pass(first["known"] + (np.float32(mv2),), 0, 0, False), True
    except _HostFile as e:                                                   # (the pass's sink has been closed on the way out)
        return host_path(be, e.args[0])
    info = dict(clipped_samples=last["clipped"], columns=last["columns"], windows=last["windows"], path="device", skipped=first["skipped"], samples=last["samples"],
                too_big=last["too_big"], too_small=last["clipped"] - last["too_big"], redone=redone, ended=last["ended"])
    if graph:
        info["graph"] = first["graph"]
    ms = dev.total_ms()
    if ms is not None:
        info["ms"] = ms
    return last["hdr"], last["out"], info


def read_csv_device(path: str, ntrks: int = 9, mode: int = tbin.MODE_NRZI, bpi: float = 0.0, ips: float = 0.0, order: str | None = None,
                    invert: bool = False, scale: float = 1.0, subsample: int = 1, maxvolts: float = 0.0, descr: str = "",
                    window_bytes: int = 1 << 28, device="cuda:0", _lib_path=None, _backend=None, _preread_rows: int | None = None, _timing: bool = False,
                    skip: int = 0, starttime: float = 0.0, endtime: float = 0.0, stopaft: int | None = None, graph: int = 0, redo: bool = False):
    """read_csv with the conversion on the device -> (TbinHeader, rows[n, ntrks] int16 ON THE DEVICE - contiguous, 16-byte aligned, what pipeline.decode_tape and
    FrontEnd.scan take -, info = read_csv's and windows, path).  Header, rows and info are read_csv's, field for field and code for code, with all its options.

    The file is read once per pass, in windows of window_bytes cut on line boundaries (the bytes behind a window's last complete line are carried to the front
    of the next one, on the device), and every byte crosses PCIe once.  The survey is rt_csv_survey's: two title lines, the peak of at most a million - 1 data
    lines (rtfe_csv_peak), the period from the first and the last surveyed timestamp (the two numbers the host parses); it always starts at the third line,
    whatever is skipped.  The windows that hold the surveyed lines stay resident until the full scale is known and they are parsed (rtfe_csv_parse); behind
    them two windows of text are resident at a time.  The window options choose the lines by convert_window's rule - sample j is raw data line
    K + j * subsample + subsample - 1 - and reading stops with the window in which -stopaft / -endtime end the pass.  graph: rtfe_csv_graph runs behind
    every rtfe_csv_parse, on the same lines, into bins that stay on the device until the pass is over.  redo: a pass that clipped is run again (the file is
    read again) with the full scale sized by the first pass's peak, which rtfe_csv_graph has kept.
    A file the host would read differently - a line longer than fgets(line, 400) returns whole, a line longer than a window, a negative first timestamp - is
    handed to read_csv: path = "host", the result is the host's, uploaded.  _lib_path / _backend / _preread_rows / _timing: hooks for the tests and tools/."""
    common = dict(ntrks=ntrks, mode=mode, bpi=bpi, ips=ips, order=order, invert=invert, scale=scale, subsample=subsample, maxvolts=maxvolts, descr=descr,
                  _preread_rows=_preread_rows, skip=skip, starttime=starttime, endtime=endtime, stopaft=stopaft, graph=graph, redo=redo)

    def host_path(be, nwindows):
        hdr, rows, info = read_csv(path, **common)
        return hdr, be.rows(rows), dict(info, windows=nwindows, path="host")
    return _device_convert(path, lambda dev: _ResidentSink(dev, ntrks), host_path, window_bytes=window_bytes, device=device, _lib_path=_lib_path, _backend=_backend,
                           _timing=_timing, **common)


def convert_csv_device(csv_path: str, tbin_path: str, graph_path: str | None = None, times=None, ntrks: int = 9, mode: int = tbin.MODE_NRZI, bpi: float = 0.0,
                       ips: float = 0.0, order: str | None = None, invert: bool = False, scale: float = 1.0, subsample: int = 1, maxvolts: float = 0.0,
                       descr: str = "", skip: int = 0, starttime: float = 0.0, endtime: float = 0.0, stopaft: int | None = None, graph: int = 0, redo: bool = False,
                       window_bytes: int = 1 << 28, device="cuda:0", _lib_path=None, _backend=None, _preread_rows: int | None = None, _timing: bool = False):
    """convert_csv with the conversion on the device, file to file: the same two files, byte for byte, and the same (TbinHeader, info) with windows and path.
    read_csv_device's window loop with a sink in place of the growing buffer: a window's rows are made in one of two device buffers, copied to one of two
    page-locked buffers on a copy stream and written by a writer thread while the next window is read, uploaded and parsed.  Resident at any time: the
    survey's text windows until the full scale is known, then two windows of text and two of rows (and the graph's bins) - a capture of any length converts.
    -redo runs the loop again and writes the .tbin again.  A file the device path hands to the host is convert_csv's: path = "host"."""
    if graph and graph_path is None:
        graph_path = (tbin_path[:-5] if tbin_path.endswith(".tbin") else tbin_path) + ".graph.csv"
    common = dict(ntrks=ntrks, mode=mode, bpi=bpi, ips=ips, order=order, invert=invert, scale=scale, subsample=subsample, maxvolts=maxvolts, descr=descr,
                  _preread_rows=_preread_rows, skip=skip, starttime=starttime, endtime=endtime, stopaft=stopaft, graph=graph, redo=redo)

    def host_path(be, nwindows):
        hdr, info = convert_csv(csv_path, tbin_path, graph_path=graph_path, times=times, **common)
        return hdr, None, dict(info, windows=nwindows, path="host")
    hdr, _, info = _device_convert(csv_path, lambda dev: _FileSink(dev, ntrks, tbin_path, times), host_path, window_bytes=window_bytes, device=device,
                                   _lib_path=_lib_path, _backend=_backend, _timing=_timing, **common)
    if graph and info["path"] == "device":
        mx = np.ascontiguousarray(info["graph"][1], dtype=np.float32)
        rc = _lib().rt_csv_graph_write(graph_path.encode(), int(graph), mx.ctypes.data, int(mx.shape[0]))
        if rc != 0:
            raise OSError(f"cannot write {graph_path} ({rc})")
    if times is not None and info["path"] == "device":
        hdr = dataclasses.replace(hdr, times=tuple(times))
    return hdr, info
