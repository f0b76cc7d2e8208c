"""The interpreted text dump of a tape (the reference's -textfile and -tapread, src/textfile.c and src/tapread.c): the file a person opens to see what
is on a tape - every record's bytes as hex or octal numbers and / or as characters of one of thirteen codes, in the style of a memory dump.

  TextOptions        -hex / -octal / -octal2, -ascii / -ebcdic / ..., -linesize=, -dataspace=, -linefeed
  text_name          "<base>.<num>.<char>.txt"
  read_tap           the items of a SIMH .tap file: records, tape marks, the reader's messages
  write_text         -tapread on the host (csrc/host/rt_tapread.c, rt_textfile.c)
  write_text_device  the same file with the body made on the device (rtfe_text_format, csrc/rtfe_textfile.hip), window by window

decode_tape(..., textfile=TextOptions(...)) writes the verbose layout beside the .tap while it decodes (pipeline.py)."""
from __future__ import annotations

import ctypes as C
import os
import queue
import threading
import time
from dataclasses import dataclass

import numpy as np

from . import csvin, frontend

HERE = os.path.dirname(os.path.abspath(__file__))
NUMS = ("none", "hex", "octal", "octal2")
CHARS = ("none", "bcd", "ebcdic", "ascii", "b5500", "sixbit", "sds", "sdsm", "flexo", "adage", "adagetape", "cdc", "univac")
RECORD, MARK, MESSAGE = 0, 1, 2
TEXT_FULL, TEXT_SCRATCH_FULL = 1, 2          # RTFE_TEXT_FULL, RTFE_TEXT_SCRATCH_FULL
ITEM = np.dtype([("offset", "<u8"), ("length", "<u4"), ("kind", "<u2"), ("flag", "<u2")])


class TapFormatError(ValueError):
    """The .tap image is one the reference stops on with a fatal error; .items are the ones in front of it, .status which error."""

    def __init__(self, msg, status, items=None):
        super().__init__(msg)
        self.status, self.items = status, items


@dataclass
class TextOptions:
    """num: None / "hex" / "octal" / "octal2"; char: None or one of CHARS; linesize 4..400 (0: 32 with both a number and a character type, otherwise
    64); dataspace 0..400: a blank behind every so many bytes of numbers (None: 2 under octal2, otherwise 0); linefeed: a 0x0a starts a new line."""
    num: str | None = None
    char: str | None = None
    linesize: int = 0
    dataspace: int | None = None
    linefeed: bool = False


class _Opts(C.Structure):
    _fields_ = [("numtype", C.c_int), ("chartype", C.c_int), ("linesize", C.c_int), ("dataspace", C.c_int), ("linefeed", C.c_int), ("ntrks", C.c_int)]


class _Out(C.Structure):
    _fields_ = [("bytes", C.c_uint64), ("lines", C.c_uint64), ("stretches", C.c_uint64), ("flags", C.c_uint32), ("pad", C.c_uint32)]


def c_options(opts: TextOptions, ntrks: int = 9) -> _Opts:
    num, char = (opts.num or "none").lower(), (opts.char or "none").lower()
    if num not in NUMS or char not in CHARS:
        raise ValueError(f"text options: no number type {opts.num!r} or character type {opts.char!r}")
    if opts.linesize and not 4 <= opts.linesize <= 400:
        raise ValueError(f"linesize {opts.linesize}: 4 .. 400")
    if opts.dataspace is not None and not 0 <= opts.dataspace <= 400:
        raise ValueError(f"dataspace {opts.dataspace}: 0 .. 400")
    return _Opts(NUMS.index(num), CHARS.index(char), int(opts.linesize), -1 if opts.dataspace is None else int(opts.dataspace), int(bool(opts.linefeed)), int(ntrks))


_lib_cache = []


def _lib():
    if not _lib_cache:
        lib = C.CDLL(os.path.join(HERE, "librtdecode.so"))
        lib.rt_text_name.argtypes = [C.c_char_p, C.POINTER(_Opts), C.c_char_p, C.c_size_t]
        lib.rt_tap_items.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int64, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
        lib.rt_tap_items.restype = C.c_int64
        lib.rt_tapread_write.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.POINTER(_Opts), C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
        lib.rt_tapread_write.restype = C.c_longlong
        lib.rt_text_new.argtypes = [C.c_char_p, C.POINTER(_Opts), C.c_int, C.c_char_p]
        lib.rt_text_new.restype = C.c_void_p
        lib.rt_text_open_now.argtypes = [C.c_void_p]
        lib.rt_text_body.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.rt_text_count_items.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        lib.rt_text_tapemark.argtypes = [C.c_void_p, C.c_double]
        lib.rt_text_message.argtypes = [C.c_void_p, C.c_char_p]
        lib.rt_text_close.argtypes = [C.c_void_p, C.c_int]
        lib.rt_text_close.restype = C.c_longlong
        _lib_cache.append(lib)
    return _lib_cache[0]


def _created(created) -> bytes:
    """What stands behind "on " in the title: ctime's format.  created: such a string, seconds since the epoch, or None for now."""
    if created is None:
        created = time.time()
    if not isinstance(created, (str, bytes)):
        created = time.ctime(created)
    created = created.encode() if isinstance(created, str) else created
    return created if created.endswith(b"\n") else created + b"\n"


def text_name(base: str, opts: TextOptions) -> str:
    """The name the reference gives the text file of <base> (src/textfile.c:192-196): g.hex.EBCDIC.txt, g.octal2.flexo.txt, g.ASCII.txt, g.txt."""
    buf = C.create_string_buffer(2048)
    if _lib().rt_text_name(os.fsencode(base), C.byref(c_options(opts)), buf, len(buf)) != 0:
        raise ValueError("text_name: bad options, or the name is too long")
    return os.fsdecode(buf.value)


def _image(tap):
    if isinstance(tap, (bytes, bytearray, memoryview)):
        return np.frombuffer(tap, np.uint8).copy()            # (writable: the device upload takes it as it is)
    if isinstance(tap, np.ndarray):
        return np.ascontiguousarray(tap, np.uint8)
    return np.fromfile(tap, np.uint8)


def _items(img):
    lib = _lib()
    st, err = C.c_int(), C.create_string_buffer(200)
    n = lib.rt_tap_items(img.ctypes.data, img.size, None, 0, C.byref(st), err, len(err))
    items = np.zeros(max(int(n), 1), ITEM)
    lib.rt_tap_items(img.ctypes.data, img.size, items.ctypes.data, n, C.byref(st), err, len(err))
    return items[:n], st.value, err.value.decode()


def read_tap(path):
    """The items of a .tap file (a path, or its bytes), in order: a structured array of offset (where the record's data lie in the file), length, kind
    (RECORD / MARK / MESSAGE) and flag (a record's error bit; which message).  An image the reference dies on raises TapFormatError (with the items in
    front of the error)."""
    items, status, err = _items(_image(path))
    if status:
        raise TapFormatError(err, status, items)
    return items


def write_text(tap_path, base: str, opts: TextOptions, ntrks: int = 9, created=None):
    """`readtape -tapread <options> <base>` on the host: the text file text_name(base, opts) of the .tap file tap_path (a path, or the bytes).  created:
    the title's date (see _created) - give it and two runs compare byte for byte.  ntrks 7 prints octal bytes with two digits.  An image the reference
    dies on raises TapFormatError after the file was left as the reference leaves it (no trailer).  -> dict(name=, bytes=)."""
    img = _image(tap_path)
    st, err = C.c_int(), C.create_string_buffer(200)
    n = _lib().rt_tapread_write(img.ctypes.data, img.size, os.fsencode(base), C.byref(c_options(opts, ntrks)), _created(created), C.byref(st), err, len(err))
    if n == -2:
        raise ValueError("write_text: bad options")
    if n < 0:
        raise OSError(f"cannot write {text_name(base, opts)}")
    if st.value:
        raise TapFormatError(err.value.decode(), st.value)
    return dict(name=text_name(base, opts), bytes=int(n))


def _windows(items, window_bytes):
    """Slices of the item table: whole items, about window_bytes of record data each (a record is never split)."""
    n = len(items)
    if n == 0:
        return []
    ends = np.cumsum(items["length"].astype(np.int64) + 16)                   # (an item without data still takes its line)
    cuts, lo = [], 0
    while lo < n:
        hi = int(np.searchsorted(ends, (ends[lo - 1] if lo else 0) + window_bytes, side="right"))
        hi = max(hi, lo + 1)
        cuts.append((lo, min(hi, n)))
        lo = min(hi, n)
    return cuts


def write_text_device(tap_path, base: str, opts: TextOptions, ntrks: int = 9, created=None, window_bytes: int = 8 << 20, _lib_path=None, _backend=None):
    """write_text with the body made on the device: the file is write_text's, byte for byte.

    The image is read by the host's reader (read_tap's table) and uploaded whole; windows of whole records - about window_bytes of record data each - go
    through rtfe_text_format into one of two resident text buffers: window k is formatted while window k - 1 is copied to page-locked memory on a copy stream
    and a writer thread puts window k - 2 into the file.  The title and the trailer are the host writer's.  The list of block sizes (no number and no
    character type) is refused: write_text makes it.  An image the reference dies on raises TapFormatError after the items in front of the error were written.
    -> dict(name=, bytes=, items=, lines=, windows=, ms=dict(upload=, format=, copy=  by stream events (None under the emulator), write= the writer
    thread's time in the file, total= wall clock))."""
    t_enter = time.perf_counter()
    be = _backend or frontend.TorchBackend()
    torch = getattr(be, "torch", None)
    lib = frontend._load_library(_lib_path)
    hlib = _lib()
    o = c_options(opts, ntrks)
    dopts = (C.c_int * 7)(o.numtype, o.chartype, o.linesize, o.dataspace, o.linefeed, o.ntrks, 0)
    img = _image(tap_path)
    items, status, err = _items(img)
    items = np.ascontiguousarray(items)
    if int(window_bytes) < 1:
        raise ValueError(f"window_bytes {window_bytes}: at least 1")
    wins = _windows(items, int(window_bytes))

    def lf_count(lo, hi):
        if not o.linefeed:
            return 0
        a, b = int(items["offset"][lo]), int(items["offset"][hi - 1]) + int(items["length"][hi - 1])
        return int(np.count_nonzero(img[a:b] == 10))

    def piece(lo, hi):
        return items[lo:hi].ctypes.data if hi > lo else None

    lfs = [lf_count(lo, hi) for lo, hi in wins]
    if lib.rtfe_text_format_scratch_bytes(None, 0, 0, dopts) == 0:                            # (every refusal comes before the file is touched)
        raise ValueError(f"rtfe_text_format refused: {lib.rtfe_last_error().decode()}")
    caps = [int(lib.rtfe_text_format_max_bytes(piece(lo, hi), hi - lo, nlf, dopts)) for (lo, hi), nlf in zip(wins, lfs)]
    scr = [int(lib.rtfe_text_format_scratch_bytes(piece(lo, hi), hi - lo, nlf, dopts)) for (lo, hi), nlf in zip(wins, lfs)]
    if any(s == 0 for s in scr):
        raise ValueError(f"rtfe_text_format refused: {lib.rtfe_last_error().decode()}")
    ctx = hlib.rt_text_new(os.fsencode(base), C.byref(o), 1, _created(created))
    if not ctx:
        raise ValueError("write_text_device: bad options")
    if hlib.rt_text_open_now(ctx) != 0:
        hlib.rt_text_close(ctx, 0)
        raise OSError(f"cannot write {text_name(base, opts)}")
    dev = csvin._Dev(be, False)
    ms = dict(upload=None, format=None, copy=None, write=0.0, total=None)
    lines = 0
    try:
        t0 = time.perf_counter()
        if torch is not None:
            d_img = torch.from_numpy(img).to(be.device) if img.size else be.empty(16)
            d_items = torch.from_numpy(items.view(np.uint8)).to(be.device) if len(items) else be.empty(16)
            be.sync()
            ms["upload"] = (time.perf_counter() - t0) * 1e3
        else:
            d_img, d_items = dev.alloc(img.size), dev.alloc(items.nbytes)
            d_img[:img.size] = img
            d_items[:items.nbytes] = items.view(np.uint8)
        cap = max(caps, default=0)
        text = [dev.alloc(cap + 16) for _ in range(min(2, len(wins)))]
        outs = [dev.alloc(32) for _ in text]
        scratch = [dev.alloc(max(scr)) for _ in text]
        fmt_events, copy_events = [], []

        def launch(k):
            lo, hi = wins[k]
            b = k % 2
            if torch is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            rc = lib.rtfe_text_format(be.ptr(d_img), img.size, piece(lo, hi), be.ptr(d_items) + 16 * lo, hi - lo, lfs[k], dopts, be.ptr(text[b]), caps[k], be.ptr(scratch[b]),
                                      int(scratch[b].shape[0]), be.ptr(outs[b]), be.stream())
            if rc != 0:
                raise ValueError(f"rtfe_text_format refused ({rc}): {lib.rtfe_last_error().decode()}")
            if torch is not None:
                e1.record()
                fmt_events.append((e0, e1))
                return e1

        def result(k):
            r = _Out.from_buffer_copy(bytes(be.to_numpy(outs[k % 2][:32], np.uint8)))      # (synchronises with window k's kernels)
            if r.flags or r.bytes > caps[k]:
                raise RuntimeError(f"rtfe_text_format: window {k} reports {r.bytes} bytes for a buffer of {caps[k]}, flags {r.flags}")
            return int(r.bytes), int(r.lines)

        def count(k):
            lo, hi = wins[k]
            hlib.rt_text_count_items(ctx, piece(lo, hi), hi - lo)

        if torch is None:
            for k in range(len(wins)):
                launch(k)
                nb, nl = result(k)
                lines += nl
                buf = np.ascontiguousarray(text[k % 2][:nb])
                hlib.rt_text_body(ctx, buf.ctypes.data, nb)
                count(k)
        elif wins:
            copy_stream = torch.cuda.Stream(be.device)
            pins = [be.pinned(cap) for _ in text]
            jobs, errors = queue.Queue(), []
            written = [threading.Event() for _ in wins]

            def writer():
                while True:
                    job = jobs.get()
                    if job is None:
                        return
                    k, nb = job
                    try:
                        if not errors:
                            t1 = time.perf_counter()
                            hlib.rt_text_body(ctx, pins[k % 2].data_ptr(), nb)
                            count(k)
                            ms["write"] += (time.perf_counter() - t1) * 1e3
                    except Exception as e:                      # (kept for the caller's thread; the windows behind it are let through unwritten)
                        errors.append(e)
                    written[k].set()
            th = threading.Thread(target=writer, daemon=True)
            th.start()
            try:
                done_fmt = launch(0)
                for k in range(len(wins)):
                    nb, nl = result(k)
                    lines += nl
                    if k >= 2:
                        written[k - 2].wait()                  # its pinned buffer is free again
                    with torch.cuda.stream(copy_stream):
                        copy_stream.wait_event(done_fmt)
                        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        c0.record(copy_stream)
                        pins[k % 2][:nb].copy_(text[k % 2][:nb], non_blocking=True)
                        c1.record(copy_stream)
                        copy_events.append((c0, c1))
                    if k + 1 < len(wins):
                        done_fmt = launch(k + 1)               # (the other device buffer: window k - 1's copy out of it was waited for below)
                    c1.synchronize()
                    jobs.put((k, nb))
            finally:
                jobs.put(None)
                th.join()
            if errors:
                raise errors[0]
        if torch is not None:
            be.sync()
            ms["format"] = float(sum(a.elapsed_time(b) for a, b in fmt_events))
            ms["copy"] = float(sum(a.elapsed_time(b) for a, b in copy_events))
    except BaseException:
        hlib.rt_text_close(ctx, 0)
        raise
    total = hlib.rt_text_close(ctx, int(status == 0))
    if total < 0:
        raise OSError(f"cannot write {text_name(base, opts)}")
    if status:
        raise TapFormatError(err, status, items)
    ms["total"] = (time.perf_counter() - t_enter) * 1e3
    return dict(name=text_name(base, opts), bytes=int(total), items=len(items), lines=lines, windows=len(wins), ms=ms)
