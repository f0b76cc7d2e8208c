"""The tape writer: a SIMH .tap image and a physical description -> the int16 rows a head would have read from that tape, resident on the device (what
pipeline.decode_tape takes as it is) or streamed into a .tbin file.  Every other path of this package goes from a waveform to bytes; this one goes back, so
that decode(write(x)) == x can be asked of any x at any size.

  WriteSpec          the description: mode, tracks, density, speed, sample time, pulse shape, noise, jitter, skew, gaps, seed
  encode             .tap (a path, its bytes, or synth's item list) -> a Plan: flux transitions on a slot grid and the table of blocks (host, C)
  encode_raw         the same from slot masks given directly, 1 .. 19 tracks
  render_host        a window of the plan's tape -> numpy int16 rows            (csrc/host/rt_tapewrite.c: the reference renderer)
  render_device      the same window -> a device tensor                         (rtfe_tape_render, csrc/rtfe_tapewrite.hip)
  write_tbin         .tap -> .tbin on the host
  write_tbin_device  .tap -> .tbin, windows rendered on the device and copied out through page-locked buffers while the next is rendered

The waveform is synth.py's model - Lorentzian pulses of alternating sign, truncated and shifted to be continuous at the cut, plus noise and jitter - with the
noise and the jitter drawn from a counter-based generator (a splitmix64 finaliser, four 16-bit fields summed: bounded at 3.46 sigma) so that host and device
agree byte for byte and a window equals the same slice of the whole tape.  With noise and jitter off the rows are synth.make_tape's.  include/rt_frontend.h
(rtfe_tape_render) states the model; DESIGN.md 4i the rest.  Whirlwind is not written: its pulse pairs do not sit on the slot grid."""
from __future__ import annotations

import ctypes as C
import os
import queue
import struct
import threading
import time
from dataclasses import dataclass, field

import numpy as np

from . import csvin, frontend, tbin, textfile

HERE = os.path.dirname(os.path.abspath(__file__))
SLOT = np.dtype([("flux", "<u4"), ("neg", "<u4")])
BLOCK = np.dtype([("first_row", "<i8"), ("rows", "<i8"), ("first_slot", "<i8"), ("nslots", "<i8")])
MAXTRKS = 19


class TapeWriteError(ValueError):
    """The description or an item of the image is one the writer refuses; .status is the C code (rt_tapewrite.h)."""

    def __init__(self, msg, status):
        super().__init__(msg)
        self.status = status


class _Spec(C.Structure):
    _fields_ = [("mode", C.c_int32), ("ntrks", C.c_int32), ("even", C.c_int32), ("reserved", C.c_int32),
                ("bpi", C.c_double), ("ips", C.c_double), ("tdelta_ns", C.c_double), ("maxvolts", C.c_double), ("amplitude", C.c_double), ("amp_slope", C.c_double),
                ("pulse_w", C.c_double), ("noise_mv", C.c_double), ("jitter", C.c_double), ("skew_cells", C.c_double * MAXTRKS),
                ("gap_samples", C.c_int64), ("seed", C.c_uint64)]


class Params(C.Structure):
    """rtfe_tape_params (include/rt_frontend.h)"""
    _fields_ = [("ntrks", C.c_int32), ("pitch_shift", C.c_int32), ("K", C.c_int32), ("reserved", C.c_int32),
                ("spb", C.c_double), ("w", C.c_double), ("edge", C.c_double), ("maxvolts", C.c_double), ("noise_mv", C.c_double), ("jitter", C.c_double),
                ("amp", C.c_double * MAXTRKS), ("skew", C.c_double * MAXTRKS), ("nkey", C.c_uint64 * MAXTRKS), ("jkey", C.c_uint64 * MAXTRKS)]


class _Plan(C.Structure):
    _fields_ = [("slots", C.c_void_p), ("nslots", C.c_int64), ("blocks", C.c_void_p), ("nblocks", C.c_int64), ("total_rows", C.c_int64), ("params", Params)]


@dataclass
class WriteSpec:
    """The tape to write.  The defaults of nrzi_spec / pe_spec / gcr_spec are synth.py's."""
    mode: int
    ntrks: int = 9
    bpi: float = 800.0
    ips: float = 50.0
    tdelta_ns: int = 1280
    maxvolts: float = 4.4
    amplitude: float = 2.5          # volts on track 0
    amp_slope: float = 0.03         # a track's amplitude is amplitude * (1 + amp_slope * track)
    pulse_w: float = 0.22           # the Lorentzian's half width, in cells
    noise_mv: float = 10.0
    jitter: float = 0.02            # sigma of a transition's place, in cells
    skew_cells: tuple = ()          # a static delay per track, in cells
    gap_samples: int = 5000
    tstart_ns: int = 1_000_000
    seed: int = 1
    even: bool = False              # NRZI: even parity

    def header(self) -> tbin.TbinHeader:
        return tbin.TbinHeader(ntrks=self.ntrks, tdelta_ns=self.tdelta_ns, maxvolts=self.maxvolts, mode=self.mode, bpi=self.bpi, ips=self.ips,
                               tstart_ns=self.tstart_ns, descr=f"written {tbin.MODE_NAMES.get(self.mode)} seed {self.seed}")

    def to_c(self) -> _Spec:
        if len(self.skew_cells) > MAXTRKS:
            raise TapeWriteError(f"{len(self.skew_cells)} skews for at most {MAXTRKS} tracks", -2)
        s = _Spec(int(self.mode), int(self.ntrks), int(bool(self.even)), 0, float(self.bpi), float(self.ips), float(self.tdelta_ns), float(self.maxvolts),
                  float(self.amplitude), float(self.amp_slope), float(self.pulse_w), float(self.noise_mv), float(self.jitter))
        for t, v in enumerate(self.skew_cells):
            s.skew_cells[t] = float(v)
        s.gap_samples, s.seed = int(self.gap_samples), int(self.seed) & 0xFFFFFFFFFFFFFFFF
        return s


def _spec(mode, seed, ntrks, kw, **defaults) -> WriteSpec:
    return WriteSpec(mode=mode, ntrks=ntrks, seed=seed, **{**defaults, **kw})


def nrzi_spec(seed: int = 1, ntrks: int = 9, **kw) -> WriteSpec:
    return _spec(tbin.MODE_NRZI, seed, ntrks, kw, bpi=800.0, ips=50.0, tdelta_ns=1280, maxvolts=4.4, pulse_w=0.22)


def pe_spec(seed: int = 1, ntrks: int = 9, **kw) -> WriteSpec:
    return _spec(tbin.MODE_PE, seed, ntrks, kw, bpi=1600.0, ips=50.0, tdelta_ns=640, maxvolts=4.4, pulse_w=0.13)


def gcr_spec(seed: int = 1, ntrks: int = 9, **kw) -> WriteSpec:
    return _spec(tbin.MODE_GCR, seed, ntrks, kw, bpi=9042.0, ips=50.0, tdelta_ns=160, maxvolts=3.3, pulse_w=0.4, amplitude=1.8, gap_samples=6000)


@dataclass
class Plan:
    """What the encoders return: the slot stream, the block table (sorted by first_row), the tape's length and the renderers' parameters."""
    spec: WriteSpec
    slots: np.ndarray               # SLOT
    blocks: np.ndarray              # BLOCK
    total_rows: int
    params: Params
    _dev: dict = field(default_factory=dict, repr=False)      # the tables on a device, by backend


_lib_cache = []


def _lib():
    if not _lib_cache:
        lib = C.CDLL(os.path.join(HERE, "librtdecode.so"))
        lib.rt_tapewrite_params.argtypes = [C.POINTER(_Spec), C.c_int, C.POINTER(Params), C.c_char_p, C.c_size_t]
        lib.rt_tapewrite_encode.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int64, C.POINTER(_Spec), C.POINTER(C.POINTER(_Plan)), C.c_char_p, C.c_size_t]
        lib.rt_tapewrite_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_Spec), C.POINTER(C.POINTER(_Plan)), C.c_char_p, C.c_size_t]
        lib.rt_tapewrite_free.argtypes = [C.POINTER(_Plan)]
        lib.rt_tapewrite_free.restype = None
        lib.rt_tapewrite_render.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(Params), C.c_int64, C.c_int64, C.c_void_p, C.c_char_p, C.c_size_t]
        _lib_cache.append(lib)
    return _lib_cache[0]


def _bind(lib):
    """rtfe_tape_render of a front-end library (librtfe.so, or the emulator's)."""
    if not hasattr(lib, "rtfe_tape_render"):
        raise RuntimeError("this build of the front-end library has no rtfe_tape_render: rebuild it")
    lib.rtfe_tape_render_span_rows.argtypes = [C.c_int]
    lib.rtfe_tape_render_span_rows.restype = C.c_int64
    lib.rtfe_tape_render.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(Params), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    return lib


def span_rows(ntrks: int, _lib_path=None) -> int:
    """The rows one workgroup of the device renderer takes (spans lie on the tape's own grid: row 0 starts one)."""
    return int(_bind(frontend._load_library(_lib_path)).rtfe_tape_render_span_rows(int(ntrks)))


def tap_image(items) -> bytes:
    """synth.make_tape's item list - ("block", payload) and ("mark",) - as a SIMH .tap image."""
    out = bytearray()
    for it in items:
        if it[0] == "mark":
            out += b"\0\0\0\0"
        elif it[0] == "block" and len(it) == 2:
            data = bytes(it[1])
            if not 0 < len(data) < (1 << 24):
                raise TapeWriteError(f"a record of {len(data)} bytes does not fit a .tap marker", -3)
            out += struct.pack("<I", len(data)) + data + b"\0" * (len(data) & 1) + struct.pack("<I", len(data))
        else:
            raise TapeWriteError(f"item {it[0]!r}: the writer takes (\"block\", payload) and (\"mark\",)", -3)
    return bytes(out + b"\xff\xff\xff\xff")


def _take(plan_p, spec) -> Plan:
    """The C plan as numpy arrays of this module's own (the C one is freed)."""
    lib = _lib()
    try:
        P = plan_p.contents
        slots = np.frombuffer(C.string_at(P.slots, P.nslots * SLOT.itemsize), SLOT).copy() if P.nslots else np.zeros(0, SLOT)
        blocks = np.frombuffer(C.string_at(P.blocks, P.nblocks * BLOCK.itemsize), BLOCK).copy() if P.nblocks else np.zeros(0, BLOCK)
        params = Params.from_buffer_copy(P.params)
        return Plan(spec=spec, slots=slots, blocks=blocks, total_rows=int(P.total_rows), params=params)
    finally:
        lib.rt_tapewrite_free(plan_p)


def encode(tap, spec: WriteSpec) -> Plan:
    """tap: the path of a .tap file, its bytes, or a list of ("block", payload) / ("mark",) items.  Records (one flagged bad in the image is data like any
    other) and tape marks become blocks of flux transitions, in the image's order, spec.gap_samples rows of gap in front of, between and behind them.
    An image the .tap reader stops on raises textfile.TapFormatError; a description or an item the format cannot carry raises TapeWriteError, naming it."""
    img = textfile._image(tap_image(tap) if isinstance(tap, (list, tuple)) else tap)
    items = textfile.read_tap(img)
    plan_p, err = C.POINTER(_Plan)(), C.create_string_buffer(400)
    rc = _lib().rt_tapewrite_encode(img.ctypes.data if img.size else None, int(img.size), items.ctypes.data if len(items) else None, len(items), C.byref(spec.to_c()),
                                    C.byref(plan_p), err, len(err))
    if rc != 0:
        raise TapeWriteError(err.value.decode(), rc)
    return _take(plan_p, spec)


def encode_raw(blocks, spec: WriteSpec) -> Plan:
    """blocks: a list of (flux, neg, ncells[, gap_before]) - per slot the mask of the tracks that have a transition there (bit t: track t) and the mask of those
    that read negative (None: every track alternates, starting positive); the block is ncells cells long (its slots lie at cell 0, 1, ... - PE: 0, 1/2, 1, ...)
    and takes ceil((ncells + 16) * samples a cell) rows behind gap_before rows of gap (default spec.gap_samples).  1 .. 19 tracks."""
    flux_all, neg_all, counts, cells, gaps = [], [], [], [], []
    for blk in blocks:
        flux = np.ascontiguousarray(blk[0], dtype=np.uint32)
        if blk[1] is None:
            before = np.bitwise_xor.accumulate(flux) ^ flux if flux.size else flux      # the tracks with an odd number of transitions in front of a slot
            neg = before & flux
        else:
            neg = np.ascontiguousarray(blk[1], dtype=np.uint32)
        if neg.shape != flux.shape or flux.ndim != 1:
            raise TapeWriteError("a block's flux and neg masks are two vectors of one length", -3)
        flux_all.append(flux), neg_all.append(neg), counts.append(flux.size), cells.append(float(blk[2]))
        gaps.append(int(blk[3]) if len(blk) > 3 else int(spec.gap_samples))
    slots = np.zeros(sum(counts), SLOT)
    if slots.size:
        slots["flux"], slots["neg"] = np.concatenate(flux_all), np.concatenate(neg_all)
    counts, cells, gaps = np.asarray(counts, np.int64), np.asarray(cells, np.float64), np.asarray(gaps, np.int64)
    plan_p, err = C.POINTER(_Plan)(), C.create_string_buffer(400)
    rc = _lib().rt_tapewrite_raw(slots.ctypes.data if slots.size else None, counts.ctypes.data, cells.ctypes.data, gaps.ctypes.data, len(counts), C.byref(spec.to_c()),
                                 C.byref(plan_p), err, len(err))
    if rc != 0:
        raise TapeWriteError(err.value.decode(), rc)
    return _take(plan_p, spec)


def _window(plan, first_row, nrows):
    first_row = int(first_row)
    nrows = plan.total_rows - first_row if nrows is None else int(nrows)
    if first_row < 0 or nrows < 0 or first_row + nrows > plan.total_rows:
        raise ValueError(f"rows {first_row} + {nrows} of a tape of {plan.total_rows}")
    return first_row, nrows


def render_host(plan: Plan, first_row: int = 0, nrows: int | None = None) -> np.ndarray:
    """Rows [first_row, first_row + nrows) of the plan's tape (default: to its end), int16 [nrows, ntrks]: the reference renderer."""
    first_row, nrows = _window(plan, first_row, nrows)
    rows = np.empty((nrows, plan.params.ntrks), np.int16)
    err = C.create_string_buffer(300)
    rc = _lib().rt_tapewrite_render(plan.slots.ctypes.data if plan.slots.size else None, plan.slots.size, plan.blocks.ctypes.data if plan.blocks.size else None,
                                    plan.blocks.size, C.byref(plan.params), first_row, nrows, rows.ctypes.data if nrows else None, err, len(err))
    if rc != 0:
        raise TapeWriteError(err.value.decode(), rc)
    return rows


def device_tables(plan: Plan, be):
    """The plan's slot stream and block table in the backend's device memory (uploaded once a plan and backend) -> (d_slots, d_blocks), None where empty."""
    if id(be) not in plan._dev:
        dev = csvin._Dev(be, False)
        out = []
        for a in (plan.slots, plan.blocks):
            d = None
            if a.size:
                d = dev.alloc(a.nbytes)
                be.upload(d, a.tobytes())
            out.append(d)
        plan._dev[id(be)] = (be, out[0], out[1])
    return plan._dev[id(be)][1:]


def render_call(lib, be, plan: Plan, first_row: int, nrows: int, ptr, stream=None) -> int:
    """rtfe_tape_render itself: the window into the device memory at ptr; -> its return code (the tests' way in; render_device raises on a refusal)."""
    d_slots, d_blocks = device_tables(plan, be)
    return lib.rtfe_tape_render(be.ptr(d_slots) if d_slots is not None else None, plan.slots.size, plan.blocks.ctypes.data if plan.blocks.size else None,
                                be.ptr(d_blocks) if d_blocks is not None else None, plan.blocks.size, C.byref(plan.params), int(first_row), int(nrows), ptr,
                                stream if stream is not None else be.stream())


def render_device(plan: Plan, first_row: int = 0, nrows: int | None = None, out=None, _lib_path=None, _backend=None):
    """render_host's rows made on the device, byte for byte: an int16 [nrows, ntrks] tensor on the GPU, queued on the current stream (nothing waits) - what
    pipeline.decode_tape takes as it is.  out: such a tensor to render into (contiguous, from a 16-byte boundary).  Under the emulator's backend a numpy array."""
    be = _backend or frontend.TorchBackend()
    lib = _bind(frontend._load_library(_lib_path))
    first_row, nrows = _window(plan, first_row, nrows)
    ntrks = plan.params.ntrks
    if out is None:
        torch = getattr(be, "torch", None)
        if torch is not None:
            out = torch.empty((nrows, ntrks), dtype=torch.int16, device=be.device)
        else:
            out = be.rows(np.zeros((nrows, ntrks), np.int16))
    if tuple(out.shape) != (nrows, ntrks):
        raise ValueError(f"out of shape {tuple(out.shape)} for {nrows} rows of {ntrks} tracks")
    rc = render_call(lib, be, plan, first_row, nrows, be.ptr(out))
    if rc != 0:
        raise TapeWriteError(f"rtfe_tape_render refused ({rc}): {lib.rtfe_last_error().decode()}", rc)
    return out


def _plan_of(tap, spec):
    return tap if isinstance(tap, Plan) else encode(tap, spec)


def write_tbin(tap, tbin_path: str, spec: WriteSpec | None = None, window_rows: int = 1 << 20):
    """The .tbin file of the tape that encode(tap, spec) describes (tap: encode's, or a Plan), rendered on the host window_rows at a time: the file
    tbin.write_tbin(path, spec.header(), all the rows) writes.  -> dict(rows=, bytes=, blocks=)."""
    plan = _plan_of(tap, spec)
    W = int(window_rows)
    if W < 1:
        raise ValueError(f"window_rows {window_rows}: at least 1")
    head = tbin.pack_header(plan.spec.header())
    with open(tbin_path, "wb") as f:
        f.write(head)
        for r in range(0, plan.total_rows, W):
            f.write(render_host(plan, r, min(W, plan.total_rows - r)).tobytes())
        f.write(struct.pack("<h", tbin.END_MARK))
    return dict(rows=plan.total_rows, bytes=len(head) + plan.total_rows * plan.params.ntrks * 2 + 2, blocks=int(plan.blocks.size))


def write_tbin_device(tap, tbin_path: str, spec: WriteSpec | None = None, window_rows: int = 1 << 23, _lib_path=None, _backend=None):
    """write_tbin with the rows rendered on the device, the same file byte for byte.  Window k is rendered into one of two device buffers while window k - 1 is
    copied to page-locked memory on a copy stream and a writer thread appends window k - 2 to the file (csvout.write_csv_device's pipeline), so the tape may be
    larger than device memory: what is resident is the slot stream, the block table and two windows.
    -> dict(rows=, bytes=, blocks=, windows=, ms=dict(render= the kernels by stream events (None under the emulator), total= wall clock))."""
    t_enter = time.perf_counter()
    plan = _plan_of(tap, spec)
    be = _backend or frontend.TorchBackend()
    torch = getattr(be, "torch", None)
    lib = _bind(frontend._load_library(_lib_path))
    W = int(window_rows)
    if W < 1:
        raise ValueError(f"window_rows {window_rows}: at least 1")
    ntrks = plan.params.ntrks
    spans = [(r, min(W, plan.total_rows - r)) for r in range(0, plan.total_rows, W)]
    dev = csvin._Dev(be, False)
    cap = min(W, max(plan.total_rows, 1)) * ntrks * 2
    bufs = [dev.alloc(cap) for _ in range(min(2, len(spans)))]
    events = []

    def launch(k):
        r, m = spans[k]
        if torch is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        rc = render_call(lib, be, plan, r, m, be.ptr(bufs[k % 2]))
        if rc != 0:
            raise TapeWriteError(f"rtfe_tape_render refused ({rc}): {lib.rtfe_last_error().decode()}", rc)
        if torch is not None:
            e1.record()
            events.append((e0, e1))
            return e1

    head = tbin.pack_header(plan.spec.header())
    done_render = launch(0) if spans else None          # (a refusal comes before the file is touched)
    with open(tbin_path, "wb", buffering=0) as f:
        f.write(head)
        if torch is None:
            for k, (r, m) in enumerate(spans):
                if k:
                    launch(k)
                f.write(bufs[k % 2][: m * ntrks * 2].tobytes())
        elif spans:
            copy_stream = torch.cuda.Stream(be.device)
            pins = [be.pinned(cap) for _ in bufs]
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
                for k, (r, m) in enumerate(spans):
                    nb = m * ntrks * 2
                    if k >= 2:
                        written[k - 2].wait()                  # its pinned buffer is free again
                    with torch.cuda.stream(copy_stream):
                        copy_stream.wait_event(done_render)
                        pins[k % 2][:nb].copy_(bufs[k % 2][:nb], non_blocking=True)
                        copied = torch.cuda.Event()
                        copied.record(copy_stream)
                    if k + 1 < len(spans):
                        done_render = launch(k + 1)            # (the other device buffer: window k - 1's copy out of it was waited for below)
                    copied.synchronize()
                    jobs.put((k, nb))
            finally:
                jobs.put(None)
                th.join()
            if errors:
                raise errors[0]
        f.write(struct.pack("<h", tbin.END_MARK))
    ms = dict(render=None, total=(time.perf_counter() - t_enter) * 1e3)
    if torch is not None:
        be.sync()
        ms["render"] = float(sum(a.elapsed_time(b) for a, b in events))
    return dict(rows=plan.total_rows, bytes=len(head) + plan.total_rows * ntrks * 2 + 2, blocks=int(plan.blocks.size), windows=len(spans), ms=ms)
