"""Streaming ingest: a .tbin file larger than the device window is decoded window by window.

Replaces the reference's read loop (two fread()s per row into a stack buffer, src/readtape.c:1405-1414) with

    disk --(reader thread, readinto)--> pinned host buffer --(hipMemcpyAsync, copy stream)--> device window
         --(rtfe_scan, compute stream)--> events --(host replay of the window's own bursts)--> piece of the .tap

A software pipeline of threads (the interpreter lock is the scarce resource: whatever runs per row or per event runs in native code):
  - the producer reads window after window into a ring of pinned buffers (rt_read_mt: native threads, positional reads) and queues each
    window's upload (copy stream) and, behind it on the scan stream, rtfe_find_end_mark (the reader's end-of-data check, on the device),
    rtfe_scan, rtfe_pack_events and the copies of the small tables into page-locked memory - `scan_contexts` windows are in flight (with
    subsample > 1 the upload goes to a raw staging buffer and rtfe_decimate_rows - thinning and end-of-data check in one - fills the window);
  - a fetcher per context waits for its window's event, copies the packed event lists to the host and hands the window to the replay pool;
  - a replay task per window runs its sub-fragments on native threads (rt_replay_run_fragments) and collects their pieces of the .tap;
  - the caller's thread concatenates the pieces in window order.
A window is a FRAGMENT in the sense of pipeline.decode_fragment: it carries a halo of the following rows, owns the bursts whose zone ends
inside it, and its .tap piece concatenates with its neighbours' (DESIGN.md 6).  PyTorch supplies the pinned allocation (hipHostMalloc), the
streams and the events; nothing here computes on the CPU except the block decoders.
"""
from __future__ import annotations

import os
import threading
import time

import numpy as np

from . import frontend, pipeline, tbin


def _payload_geometry(path):
    """(header, payload offset, whole rows in the file).  The data end at the first row whose head-0 sample is 0x8000
    (src/readtape.c:1410) - normally the lone int16 behind the last row; the reader also looks for it inside every window."""
    hdr, off = tbin.read_header(path)
    nrows = (os.path.getsize(path) - off) // (2 * hdr.ntrks)
    return hdr, off, int(nrows)


class _All:
    """Several futures waited for as one (a device window is free again when all replays of its sub-fragments are done)."""

    def __init__(self, futs):
        self.futs = futs

    def result(self):
        for f in self.futs:
            f.result()


def _prepass_needs(hdr, cfgkw, deskew):
    """(density to detect, delays to calibrate) - what the header and the caller's configuration leave open."""
    need_bpi = hdr.mode != tbin.MODE_GCR and not hdr.bpi > 0 and not cfgkw.get("bpi")
    need_skew = bool(deskew) and cfgkw.get("skew") is None and hdr.mode != tbin.MODE_PE      # "-deskew option is ignored for PE", src/readtape.c:1677
    return need_bpi, need_skew


def _settle(hdr, full, opts, cfgkw, need_bpi, need_skew, make_fe, run, log_path=None):
    """The two pre-passes in the reference's order (src/readtape.c:1656-1717): the density, then the delays with that density -> cfgkw with "bpi" / "skew".
    run(what, fn): calls fn(rows, more_rows) on the rows the caller has - the streaming reader's growing prefix, a rank's resident share - and returns
    its answer (never None: an undecided pre-pass is the caller's to resolve or to refuse)."""
    invert, find_zeros, differentiate = (bool(cfgkw.get(k, False)) for k in ("invert", "find_zeros", "differentiate"))

    def options(bpi):
        return pipeline._Options(mode=hdr.mode, ntrks=hdr.ntrks, bpi=bpi, ips=hdr.ips or 50.0, specified_parity=0 if opts.even_parity else 1, revparity=opts.revparity,
                                 do_correction=int(opts.correct), find_zeros=int(find_zeros), do_differentiate=int(differentiate),
                                 multiple_tries=int(opts.multiple_tries), tap_format=1, add_parity=0, verbose=int(opts.verbose))

    cfgkw = dict(cfgkw)
    if need_bpi:
        cfgkw["bpi"] = run("density detection", lambda rows, more: pipeline.detect_density(
            hdr, rows, full, options(0.0), make_fe, invert=invert, first_prefix_rows=max(1, int(rows.shape[0])), more_rows=more, log_path=log_path))
    if need_skew:
        rest = {k: v for k, v in cfgkw.items() if k not in ("invert", "find_zeros", "differentiate", "skew")}
        bpi = frontend.FrontEndConfig.from_header(hdr, **({"bpi": cfgkw["bpi"]} if "bpi" in cfgkw else {})).bpi
        cfgkw["skew"] = run("-deskew calibration", lambda rows, more: pipeline.calibrate_deskew(
            hdr, rows, full, options(bpi), make_fe, invert=invert, find_zeros=find_zeros, differentiate=differentiate,
            first_prefix_rows=max(1, int(rows.shape[0])), more_rows=more, log_path=log_path, append=bool(need_bpi and log_path), **rest))
    return cfgkw


def _prepasses(hdr, fd, off, nrows, nth, full, opts, cfgkw, deskew, prepass_rows, device, fe_factory=None, backend=None, lib=None, log_path=None):
    """What the reference settles before its main pass (src/readtape.c:1656-1717), on a prefix of the file: the density of a header without one, then the
    -deskew delays with that density - pipeline.detect_density / calibrate_deskew, which the resident decode runs on its whole tape.  -> cfgkw with what they
    found ("bpi", "skew"); unchanged, and nothing read or launched, where neither is asked for.  off: the payload behind the skipped rows; nrows: used rows.
    fe_factory / backend / lib: the front ends, the memory and the library of the prefix (default: the GPU's; shard.decode_file_sharded hands its own on,
    tests/cpu_emul's included - with a backend of the caller's the prefix is host arrays)."""
    need_bpi, need_skew = _prepass_needs(hdr, cfgkw, deskew)
    if not (need_bpi or need_skew) or nrows <= 0:
        return cfgkw
    if need_bpi and hdr.mode != tbin.MODE_NRZI:
        pipeline.detect_density(hdr, None, full, None, None)      # (raises what the resident decode raises: density detection is NRZI's)
    import torch
    ntrks = hdr.ntrks
    on_host = backend is not None
    be, lib, dlib = backend or frontend.TorchBackend(device), lib or frontend._load_library(), pipeline._load_decode_lib()
    make_fe = fe_factory or (lambda c: frontend.FrontEnd(c, device=device))

    def prefix(want):
        """the used rows [0, want) on the device, cut at the end marker -> (rows, whether the tape goes on behind them)"""
        host = torch.empty((want * nth, ntrks), dtype=torch.int16, pin_memory=not on_host)
        if dlib.rt_read_mt(fd, host.numpy().ctypes.data, off, want * nth * 2 * ntrks, 4) != 0:
            raise IOError("short read")
        if on_host:
            d_raw, rows = host.numpy(), torch.empty((want, ntrks), dtype=torch.int16).numpy()
        else:
            d_raw, rows = host.to(torch.device(device), non_blocking=True), torch.empty((want, ntrks), dtype=torch.int16, device=torch.device(device))
        d_mark = be.empty(16)
        frontend.decimate_rows(lib, be, d_raw, want * nth, nth - 1, nth, rows, d_mark)      # (step 1: a copy and the end-of-data check)
        m = int(be.to_numpy(d_mark, np.int64)[0])
        used = want if m == np.iinfo(np.int64).max else min(want, m // nth)
        return rows[:used], used == want and want < nrows

    def run(what, fn):
        want = min(nrows, max(1024, prepass_rows))
        while True:
            try:
                rows, more = prefix(want)
                got = fn(rows, more)
            except torch.cuda.OutOfMemoryError as e:
                raise RuntimeError(f"{what}: undecided on the longest prefix the device holds (a prefix of {want} rows does not fit): nothing was decoded") from e
            if got is not None:
                return got
            del rows
            want = min(nrows, want * 4)                    # (None only with more rows behind the prefix: want < nrows)

    return _settle(hdr, full, opts, cfgkw, need_bpi, need_skew, make_fe, run, log_path=log_path)


def plan_windows(raw_rows, window_rows, halo_rows, subsample=1, skip=0, ramp=True):
    """The windows of a payload of `raw_rows` rows -> [(lo, hi, raw_lo, raw_hi), ...].
    Windows are planned in USED rows - the rows the scans see: of every `subsample` raw rows behind the first `skip`, the last (src/readtape.c:1407-1424,
    1634-1641) - so that the cuts stay on the 1024-row grid the fragments' ownership rule stands on.  Window k owns the used rows [lo, hi)
    and is scanned with a halo of up to halo_rows further ones; the raw rows it is made of are [raw_lo, raw_hi) = [skip + lo * n, skip + min(hi + halo_rows,
    used rows) * n).  An incomplete group of raw rows at the end of the payload is no used row.
    ramp: the first two windows are a quarter and a half of window_rows (the pipeline fills sooner), and the last two windows' worth of rows go as a
    half, a quarter and two eighths of what is left (it drains sooner) - for windows of 2^20 rows and more."""
    assert window_rows % 1024 == 0 and window_rows > 0 and halo_rows >= 0 and subsample >= 1 and skip >= 0
    n = int(subsample)
    nrows = max(0, int(raw_rows) - int(skip)) // n
    spans, lo = [], 0
    sizes = [window_rows // 4 & ~1023, window_rows // 2 & ~1023] if (ramp and window_rows >= (1 << 20) and nrows > 2 * window_rows) else []
    while lo < nrows:
        w = sizes.pop(0) if sizes else window_rows
        if ramp and not sizes and window_rows >= (1 << 20) and len(spans) >= 2 and nrows - lo <= 2 * window_rows and nrows - lo > (1 << 20):
            # ... and drains sooner behind short last windows: what follows the last upload - its scan, its fetch, its replay - is in nobody's shadow.  The last
            # two windows' worth of rows go as a half, a quarter and two eighths of what is left.
            rest = nrows - lo
            for frac in (2, 4, 8):
                w2 = max(1 << 18, rest // frac & ~1023)
                if lo + w2 < nrows:
                    spans.append((lo, lo + w2)); lo += w2
            spans.append((lo, nrows)); lo = nrows
            break
        spans.append((lo, min(nrows, lo + w)))
        lo += w
    return [(lo, hi, skip + lo * n, skip + min(nrows, hi + halo_rows) * n) for lo, hi in spans]


def decode_file_streaming(path, tap_path, window_rows=1 << 24, halo_rows=1 << 17, opts: pipeline.DecodeOptions | None = None, cfgkw=None,
                          device="cuda:0", replay_threads: int = 1, read_threads: int = 4, replay_split: int = 1, scan_contexts: int = 3, ramp: bool = True,
                          subsample: int = 1, skip: int = 0, deskew: bool = False, skew=None, prepass_rows: int = 1 << 22,
                          peakstats: bool = False):
    """Decodes the .tbin file `path` to the SIMH file `tap_path` through device windows of `window_rows` rows (a multiple of 1024).
    Returns statistics incl. the end-to-end rate (disk -> .tap), the time spent in the host replay and the rows the halos re-read.
    replay_threads > 1: the windows' host replays run side by side (fragments are independent: each has its own decoder context
    and writes its own piece of the .tap; the pieces are concatenated in window order).  A window's device buffer is kept until
    its replay is done (exact rescans read it), so replay_threads + 2 device windows are held.
    replay_split > 1: a window's bursts are replayed as that many sub-fragments side by side (cut at burst boundaries, exactly as the
    windows themselves are); the last two windows - what the pipeline drains into - as four times as many.
    scan_contexts: scans in flight (a context = a front end with its workspace and output buffers; a context is free again once its window's
    results have been fetched).  ramp: the first two windows are a quarter and a half of `window_rows` (the pipeline fills sooner).
    The reference's reader options (statistics: rows = the USED rows decoded, raw_rows = the payload rows they stand for, the skipped ones included):
      skip       the first `skip` rows of the payload are not part of the tape: the time base does not advance over them and an end marker among them is not
                 looked at (src/readtape.c:1634-1641) - the decode of rows[skip:].
      subsample  n: of every n raw rows behind the skip the last one is used, the time base advances by the header's tdelta per used row, and the data end at
                 the first RAW row whose head-0 sample is 0x8000, used or not (src/readtape.c:1407-1424) - the decode of rows[skip:][n - 1::n].  Windows,
                 halos and window_rows count used rows (plan_windows); each window is uploaded raw and thinned on the device (rtfe_decimate_rows, which
                 also is its end-of-data check).  Memory: the pinned buffers and scan_contexts + 1 raw device staging buffers hold n times a window's
                 rows; the device windows themselves do not grow.
      density    a header without bpi (NRZI): pipeline.detect_density on a prefix of the used rows; PE raises what the resident decode raises.
      deskew     pipeline.calibrate_deskew on a prefix, with the detected density, unless `skew` (the delays, in samples per track) is given or the mode is PE.
    The pre-passes run before the pipeline starts, on the first prepass_rows used rows read the reader's way (pinned, uploaded, thinned), with the main pass's
    invert / find_zeros / differentiate and no delays.  A pre-pass whose stopping rule is not met inside the prefix gets a prefix four times as long, up
    to the whole tape; if that does not fit the device a RuntimeError says so (nothing is ever streamed with a guessed density or partial delays).
    statistics["bpi"], ["skew"]: what the scans ran with.  With the defaults and a header that states its density nothing of this costs a launch or a buffer."""
    pipeline.refuse_peakstats(peakstats, "ingest.decode_file_streaming")
    return _decode_file(path, tap_path, window_rows, halo_rows, opts, cfgkw, device, replay_threads, read_threads, replay_split, scan_contexts, ramp,
                        subsample, skip, deskew, skew, prepass_rows, None)


class _Windows:
    """What decode_file_windows adds to the streaming reader: the header as the command line overrides it, the parameter sets of a .parms text, the log the
    pre-passes begin, and the finisher (pipeline.Finisher) the windows' journals go to - made on the caller's thread once the configuration is settled."""

    def __init__(self, out, hdr_overrides, parms_text):
        self.out, self.parms_text = out, parms_text
        self.hdr_overrides = {{"order": "trkorder"}.get(k, k): v for k, v in (hdr_overrides or {}).items() if v is not None}
        self.log_path = out.get("log_path")

    def header(self, hdr):
        import dataclasses
        return dataclasses.replace(hdr, **self.hdr_overrides) if self.hdr_overrides else hdr

    def parmsets(self, hdr, opts):
        nsets = opts.nparmsets or (15 if opts.multiple_tries else 1)
        if not self.parms_text:
            return pipeline.default_parmsets(hdr.mode, nsets)
        arr = (pipeline._Parms * 15)()
        n = pipeline._load_decode_lib().rt_parse_parms_text(hdr.mode, self.parms_text.encode(), arr)
        if n <= 0:
            raise ValueError("bad .parms text")
        return [arr[i] for i in range(n)][:nsets]

    def finisher(self, hdr, cfg, full, opts, began):
        return pipeline.Finisher(hdr, cfg, full, opts, append=began, **self.out)


class _Consumed:
    """A device window of the windowed decode stays as it is until the finisher has taken its journals (a fragment whose neighbour's last block ran into it is
    replayed again, from the window's rows): what launch() waits for besides the window's replays."""

    def __init__(self, waited):
        self.ev, self.waited = threading.Event(), waited

    def result(self):
        t0 = time.perf_counter()
        self.ev.wait()
        self.waited[0] += time.perf_counter() - t0


def _decode_file(path, tap_path, window_rows, halo_rows, opts, cfgkw, device, replay_threads, read_threads, replay_split, scan_contexts, ramp,
                 subsample, skip, deskew, skew, prepass_rows, sink):
    """decode_file_streaming's pipeline; sink: None, or decode_file_windows' _Windows - the fragments journal their blocks and one finisher puts them out."""
    import queue
    import torch
    assert window_rows % 1024 == 0
    t_enter = time.perf_counter()
    opts = opts or pipeline.DecodeOptions()
    hdr, off, raw_rows = _payload_geometry(path)
    if sink:
        hdr = sink.header(hdr)
    if hdr.mode == tbin.MODE_WW:
        raise NotImplementedError("Whirlwind tapes are one chain (no independent fragments): read the file and use pipeline.decode_tape_ww")
    nth, skip = int(subsample), int(skip)
    if nth < 1 or skip < 0:
        raise ValueError(f"subsample {subsample} (at least 1), skip {skip} (not negative)")
    ntrks = hdr.ntrks
    plan = plan_windows(raw_rows, window_rows, halo_rows, nth, skip, ramp)
    spans = [(lo, hi) for lo, hi, _, _ in plan]
    off += skip * 2 * ntrks                               # (the payload, from here on: what lies behind the skipped rows)
    nrows = max(0, raw_rows - skip) // nth               # used rows: every row index below counts these
    gpu_mark = os.environ.get("RTFE_PACK_EVENTS") != "0" and not os.environ.get("RT_INGEST_HOST_MARK")
    if nth > 1 and not gpu_mark:
        raise NotImplementedError("subsample > 1: the windows' end-of-data check is the thinning kernel's (unset RT_INGEST_HOST_MARK / RTFE_PACK_EVENTS=0)")
    full = sink.parmsets(hdr, opts) if sink else pipeline.default_parmsets(hdr.mode, opts.nparmsets or (15 if opts.multiple_tries else 1))
    dev = torch.device(device)
    cfgkw = dict(cfgkw or {})
    if skew is not None:
        cfgkw["skew"] = [int(x) for x in skew]
    fd = os.open(path, os.O_RDONLY)
    finisher = None
    try:
        began = bool(sink and sink.log_path and nrows > 0 and any(_prepass_needs(hdr, cfgkw, deskew)))      # (the pre-passes begin the log, the finisher continues it)
        cfgkw = _prepasses(hdr, fd, off, nrows, nth, full, opts, cfgkw, deskew, int(prepass_rows), device, log_path=sink.log_path if sink else None)
        cfg = frontend.FrontEndConfig.from_header(hdr, parmsets=pipeline.frontend_parmsets(full), **cfgkw)
    except BaseException:
        os.close(fd)
        raise
    nctx = max(2, int(scan_contexts))
    fes = [frontend.FrontEnd(cfg, device=device) for _ in range(nctx)]      # window k is fetched while k + 1 .. are copied and scanned
    fe = fes[0]
    cap = window_rows + halo_rows
    from concurrent.futures import ThreadPoolExecutor
    nthreads = max(1, int(replay_threads))
    depth = max(2 if nthreads == 1 else nthreads + 2, nctx + 2)
    NP = nctx + 1                                         # pinned buffers: one being read into, the others being copied from / waiting for their context
    pinned = [torch.empty((cap * nth, ntrks), dtype=torch.int16, pin_memory=True) for _ in range(NP)]      # hipHostMalloc
    dwin = [torch.empty((cap, ntrks), dtype=torch.int16, device=dev) for _ in range(depth)]
    # -subsample: a window is uploaded raw into a staging buffer and thinned from there into its device window, on the scan's stream in front of the scan; the
    # staging buffer is free again when that has run (`thinned`), so there are as many as pinned buffers - the device windows, which the replays' exact
    # rescans keep reading, stay as they are
    staging = [torch.empty((cap * nth, ntrks), dtype=torch.int16, device=dev) for _ in range(NP)] if nth > 1 else None
    thinned = [torch.cuda.Event() for _ in range(NP)] if nth > 1 else None
    pool = ThreadPoolExecutor(max(2, -(-nthreads // max(1, int(replay_split))))) if nthreads > 1 else None      # a task is a window: its sub-fragments are native threads
    read_threads = max(1, int(read_threads))
    readers = ThreadPoolExecutor(read_threads) if read_threads > 1 else None
    fe_exact = frontend.FrontEnd(cfg, device=device)       # exact rescans of the replays: their own context, one at a time
    exact_lock = threading.Lock()
    copy_stream, scan_stream = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    copied = [torch.cuda.Event() for _ in range(NP)]
    dlib = pipeline._load_decode_lib()
    t_read = [0.0]
    trace = [] if os.environ.get("RT_INGEST_TRACE") else None      # (stage, window, start, end) in seconds since the timed region began
    t_base = [0.0]

    def mark(stage, k, t0):
        if trace is not None:
            trace.append((stage, k, round(t0 - t_base[0], 5), round(time.perf_counter() - t_base[0], 5)))
    data_end = [nrows]
    end_lock = threading.Lock()

    for f in fes:                                         # the end-of-data marker is looked for on the device, in front of each window's scan (rtfe_find_end_mark)
        f.pack_on_scan, f.find_end_mark = True, gpu_mark

    def read_span(arr, r0, r1, lo, check=True):
        """raw rows [lo * nth + r0, lo * nth + r1) of the payload -> arr[r0:r1]; returns the first of them (relative to lo * nth) whose head-0
        sample is the end marker, or -1 (looked for here, by the thread that has just read the rows: a strided pass over the whole window in one
        thread had become the longest stage of the pipeline)."""
        view = memoryview(arr).cast("B")[r0 * 2 * ntrks: r1 * 2 * ntrks]
        pos, done = off + (lo * nth + r0) * 2 * ntrks, 0
        while done < len(view):
            got = os.preadv(fd, [view[done: done + (1 << 30)]], pos + done)
            if got <= 0:
                raise IOError("short read")
            done += got
        if not check:
            return -1
        marks = np.flatnonzero(arr[r0:r1, 0] == tbin.END_MARK)
        return r0 + int(marks[0]) if marks.size else -1

    def read_rows(dst, lo, end, check=True):
        """the raw rows of the used rows [lo, end) of the payload -> the pinned tensor dst (positional reads: safe beside the other thread's), in
        `read_threads` pieces side by side (from the page cache one thread copies ~13 GB/s).  Returns the used rows (behind lo) in front of the first
        end marker, or -1."""
        t0 = time.perf_counter()
        arr = dst.numpy()
        n = (end - lo) * nth
        if not check:                                      # (the end marker is looked for on the device: the read is one call into native threads)
            if dlib.rt_read_mt(fd, arr.ctypes.data, off + lo * nth * 2 * ntrks, n * 2 * ntrks, read_threads) != 0:
                raise IOError("short read")
            first = -1
        elif readers is None or n * 2 * ntrks < (8 << 20):
            first = read_span(arr, 0, n, lo, check)
        else:
            step = -(-n // read_threads)
            futs = [readers.submit(read_span, arr, a, min(n, a + step), lo, check) for a in range(0, n, step)]
            hits = [h for h in (f.result() for f in futs) if h >= 0]
            first = min(hits) if hits else -1
        t_read[0] += time.perf_counter() - t0
        return first // nth if first >= 0 else -1         # (a group of nth rows that the marker cuts short is no used row)

    def read_window(k):
        lo, hi = spans[k]
        end = min(nrows, hi + halo_rows)
        t0 = time.perf_counter()
        first = read_rows(pinned[k % NP], lo, end, check=not gpu_mark)
        mark("read", k, t0)
        with end_lock:                                    # (the producer writes it while the main thread clamps a window with it)
            if first >= 0:                                # an end marker inside the payload: the tape ends there
                data_end[0] = min(data_end[0], lo + first)
            return min(end, data_end[0])

    busy = [None] * depth
    ctx_free = [threading.Semaphore(1) for _ in range(nctx)]
    stop = threading.Event()

    def launch(k, end):
        lo, hi = spans[k]
        hi = min(hi, data_end[0])
        if hi <= lo:
            return None, None, lo
        t0 = time.perf_counter()
        ctx_free[k % nctx].acquire()                      # the results of the window that used this context have been fetched
        if busy[k % depth] is not None:                   # the replay that still reads this device window
            busy[k % depth].result()
            busy[k % depth] = None
        mark("wait_ctx", k, t0)
        t0 = time.perf_counter()
        with torch.cuda.stream(copy_stream):
            if trace is not None:
                gpu_ev[("copy0", k)] = torch.cuda.Event(enable_timing=True); gpu_ev[("copy0", k)].record(copy_stream)
            if nth == 1:
                dwin[k % depth][: end - lo].copy_(pinned[k % NP][: end - lo], non_blocking=True)
            else:
                if k >= NP:
                    copy_stream.wait_event(thinned[k % NP])      # window k - NP has been thinned out of this staging buffer
                staging[k % NP][: (end - lo) * nth].copy_(pinned[k % NP][: (end - lo) * nth], non_blocking=True)
            copied[k % NP].record(copy_stream)
            if trace is not None:
                gpu_ev[("copy1", k)] = torch.cuda.Event(enable_timing=True); gpu_ev[("copy1", k)].record(copy_stream)
        mark("l_h2d", k, t0)
        scan_stream.wait_event(copied[k % NP])
        piece = dwin[k % depth][: end - lo]
        raw = (staging[k % NP][: (end - lo) * nth], nth - 1, nth, lambda: thinned[k % NP].record(scan_stream)) if nth > 1 else None
        fin = pipeline.scan_fragment(fes[k % nctx], piece, hi - lo, lo, lo == 0, hi >= data_end[0], stream=scan_stream.cuda_stream, raw=raw)
        if trace is not None:
            gpu_ev[("scan1", k)] = torch.cuda.Event(enable_timing=True); gpu_ev[("scan1", k)].record(scan_stream)
        mark("launch", k, t0)
        if trace is not None and getattr(fin.res, "launch_times", None):
            lt = fin.res.launch_times
            for name, a, b in (("l_scan", lt[0], lt[1]), ("l_pack", lt[1], lt[2]), ("l_mirror", lt[2], lt[3])) if len(lt) == 4 else ():
                trace.append((name, k, round(a - t_base[0], 5), round(b - t_base[0], 5)))
        return piece, fin, end

    launched = queue.Queue()

    def producer():
        """reads window after window into the ring of pinned buffers and queues each one's copy and scan behind its predecessor's"""
        try:
            for k, (lo, hi) in enumerate(spans):
                if stop.is_set() or lo >= data_end[0]:
                    break
                if k >= NP:
                    copied[k % NP].synchronize()           # the pinned buffer's last copy (window k - NP) has left it
                end = read_window(k)
                stats["windows_read"] = k + 1
                if stop.is_set():
                    break
                item = launch(k, end)
                if item[1] is None:
                    marks_seen[k].set()
                launched.put((k, fetchers.submit(stage2, k, item) if item[1] is not None else None))
            launched.put((None, None))
        except BaseException as e:                         # the main thread raises it
            launched.put((None, e))
        finally:
            for ev in marks_seen:                          # (windows that were never launched hold nobody up)
                if stop.is_set():
                    ev.set()

    retired = []                                          # scan contexts replaced by ones with a calibrated screen floor (closed at the end: a scan of theirs may still be in flight)
    floor_state = {"tries": 2, "floor": None}
    pieces = []                                           # per window: bytes, or the future that returns (bytes, replay stats, seconds)

    def journal_window(k, res, piece, lo, starts, stops, safes):
        """the windowed decode's replay of a window: its sub-fragments into journals -> what the finisher needs to take them (and to replay one again)"""
        t0 = time.perf_counter()
        js = [finisher.journal(first=(lo == 0 and j == 0)) for j in range(len(starts))]
        live.update(js)
        secs = pipeline.journal_fragments(hdr, cfg, fe_exact, res, piece, lo, starts, stops, js, full, opts, exact_lock=exact_lock)
        mark("replay", k, t0)
        return dict(k=k, journals=js, secs=secs, starts=starts, stops=stops, safes=safes, res=res, piece=piece, lo=lo)

    def replay(k, res, piece, lo, bound, start=None, tag=""):
        t0 = time.perf_counter()
        frag = f"{tap_path}.frag{k}{tag}"
        if start is None:
            start = 0 if lo == 0 else int(res.bursts[0]["zone_first"])
        st = pipeline.decode_fragment(hdr, cfg, fe_exact, res, piece, lo, start, bound, frag, full, opts, exact_lock=exact_lock)      # (always: the fetcher threads replay side by side on ONE exact-rescan handle - ADVICE r5)
        with open(frag, "rb") as g:
            data = g.read()
        os.remove(frag)
        mark("replay" + tag, k, t0)
        return data, st, time.perf_counter() - t0

    def replay_window(k, res, piece, lo, starts, stops):
        """-> [(bytes, replay statistics, seconds), ...] of the window's sub-fragments, in order"""
        t0 = time.perf_counter()
        frags = [f"{tap_path}.frag{k}.{j}" for j in range(len(starts))]
        sts = pipeline.decode_fragments(hdr, cfg, fe_exact, res, piece, lo, starts, stops, frags, full, opts, exact_lock=exact_lock)
        out = []
        for frag, (st, secs) in zip(frags, sts):
            with open(frag, "rb") as g:
                out.append((g.read(), st, secs))
            os.remove(frag)
        mark("replay", k, t0)
        return out

    stats = dict(rows=nrows, windows=len(spans), halo_rows_read=0, blocks=0, tapemarks=0, events_delivered=0, exact_scans=0, retries=0, replay_threads=nthreads, all_ok=True)
    t_replay = 0.0
    for f in fes:                                         # set-up, like the pinned buffers and the device windows: the scan contexts' workspaces
        f._pack_buffers(f._buffers(cap), f._buffers(cap)["cap"] // 2)
    # (and page-locked blocks for the windows' event lists in the host allocator's cache.  A window's packed events are ~1 / 40 of its arena - C2: 27 MB of events in
    #  31 - 35 MB of packed lists -, the allocator's blocks are powers of two, and a request one byte over 32 MB is a hipHostMalloc of 64 MB in the middle of the
    #  pipeline: ~12 ms during which every thread that talks to the runtime waits (round 6's trace: the producer's event wait, the fetchers).  Blocks of the NEXT power of two.)
    blk = [torch.empty(max(1 << 20, cap * ntrks * 16 // 20), dtype=torch.uint8, pin_memory=True) for _ in range(min(depth, 12))]
    del blk
    torch.cuda.synchronize(dev)
    gpu_ev = {}
    if trace is not None:
        gpu_ev["base"] = torch.cuda.Event(enable_timing=True); gpu_ev["base"].record(copy_stream); copy_stream.synchronize()
    t_start = time.perf_counter()
    t_base[0] = t_start
    total = 0
    calib_lock = threading.Lock()
    marks_seen = [threading.Event() for _ in spans]
    fin_wait = [0.0]
    consumed = [_Consumed(fin_wait) for _ in spans] if sink else None
    live = set()                                          # journals made and not yet finished or dropped
    fetchers = ThreadPoolExecutor(nctx)                    # a window's results are fetched (and its replays queued) beside its neighbours': a fetch is ~6 ms of host-side work
    fetch_streams = [torch.cuda.Stream(dev) for _ in range(nctx)]
    wait_s = [0.0]

    def stage2(k, item):
        """window k: its results to the host, its bursts to the replay threads -> the replays' futures (or results), in order"""
        piece, fin, end_k = item
        out = []
        try:
            lo, hi = spans[k]
            hi = min(hi, data_end[0])
            t0 = time.perf_counter()
            with torch.cuda.stream(fetch_streams[k % nctx]):
                res, nb, bound = fin()
            wait_s[0] += time.perf_counter() - t0
            mark("fetch", k, t0)
            if gpu_mark:
                # the window's end-of-data check came back with its tables.  The windows are looked at in order (a marker ends the tape for every window
                # behind it); a window that holds one - rows behind the data's end were scanned with it - is scanned again up to the marker.
                if k > 0:
                    marks_seen[k - 1].wait()
                try:
                    assert res.end_mark_valid
                    if lo >= data_end[0]:
                        return []
                    em = None if res.end_mark is None else res.end_mark // nth      # (the thinning kernel reports a RAW row of the window: the used rows in front of it)
                    if em is not None and em < end_k - lo:
                        with end_lock:
                            data_end[0] = min(data_end[0], lo + em)
                        end_k = min(end_k, data_end[0])
                        hi = min(hi, data_end[0])
                        if hi <= lo:
                            return []
                        piece = piece[: end_k - lo]
                        with torch.cuda.stream(fetch_streams[k % nctx]):
                            # (a marker inside this window's HALO leaves the window its own rows [lo, hi) only: it keeps its bounding burst, and the
                            #  window behind it decodes [hi, data_end) - ADVICE r5: is_last = True there decoded that range twice)
                            res, nb, bound = pipeline.scan_fragment(res.fe, piece, hi - lo, lo, lo == 0, hi >= data_end[0])()
                finally:
                    marks_seen[k].set()
            if trace is not None and getattr(res, "fetch_times", None):
                ft = res.fetch_times
                for name, a, b in (("f_wait", ft[0], ft[1]), ("f_tables", ft[1], ft[2]), ("f_events", ft[2], ft[3])):
                    trace.append((name, k, round(a - t_base[0], 5), round(b - t_base[0], 5)))
            if floor_state["tries"] > 0 and cfg.peak_detection_floor_applies():
                # The candidate screen is built for the loosest thresholds any AGC state could ask for - a learned peak height of 1 V -, and on a
                # noisy tape every wiggle above THAT becomes a record (lists outgrow their slots, the bursts are redone on the samples).  The first
                # windows say how high the tape's peaks really are: the scans behind them screen against half the smallest height a chain learned
                # (a later chain below that floor is flagged RTFE_F_SCREEN_UNDERFLOW and rescanned exactly: slower, never wrong).
                with calib_lock:
                    if floor_state["tries"] > 0:
                        floor_state["tries"] -= 1
                        st_k = res.fe.scan_stats(res)
                        if floor_state["floor"] is None:      # (what the window's own first scan estimated from its samples, k_scan_begin)
                            floor_state["floor"] = st_k.get("screen_floor_used")
                        if st_k["bursts"] > 0 and st_k["redone"] * 4 > st_k["bursts"] and st_k.get("min_learned_height"):
                            import dataclasses
                            cfg2 = dataclasses.replace(cfg, screen_floor_height=min(4.0, 0.5 * st_k["min_learned_height"]))
                            new = [frontend.FrontEnd(cfg2, device=device) for _ in range(nctx)]
                            for f in new: f._pack_buffers(f._buffers(cap), f._buffers(cap)["cap"] // 2); f.pack_on_scan, f.find_end_mark = True, gpu_mark
                            retired.extend(fes)
                            fes[:] = new                     # (the producer takes a window's context from the list when it launches it)
                            floor_state["tries"] = 0; floor_state["floor"] = cfg2.screen_floor_height
            halo = halo_rows
            while nb is None and end_k < data_end[0]:    # the last own burst runs past the halo: read more (rare; synchronous)
                halo *= 4
                stats["retries"] += 1
                end_k = min(data_end[0], hi + halo)
                host = torch.empty(((end_k - lo) * nth, ntrks), dtype=torch.int16, pin_memory=True)
                first = read_rows(host, lo, end_k)
                if first >= 0:                            # an end marker inside the longer halo: the tape ends there (src/readtape.c:1410)
                    with end_lock:
                        data_end[0] = min(data_end[0], lo + first)
                    end_k = min(end_k, data_end[0])
                piece = host[: (end_k - lo) * nth].to(dev)
                if nth > 1:                              # (-subsample: the longer window is thinned as the windows are; its marker has been looked for above)
                    wide, piece = piece, torch.empty((end_k - lo, ntrks), dtype=torch.int16, device=dev)
                    frontend.decimate_rows(fe.lib, fe.backend, wide, (end_k - lo) * nth, nth - 1, nth, piece, fe.backend.empty(16))
                    torch.cuda.current_stream(dev).synchronize()      # (`wide` goes out of scope: the allocator may hand it to another stream)
                res, nb, bound = pipeline.scan_fragment(res.fe, piece, hi - lo, lo, lo == 0, hi >= data_end[0])()
            stats["halo_rows_read"] += end_k - hi
            if res.nbursts:
                if pool:
                    # sub-fragments: cut at the zone starts of evenly spaced bursts; one task (a Python thread) per window, native threads for its sub-fragments
                    split = int(replay_split) * (4 if k + 3 >= len(spans) else (2 if k + 5 >= len(spans) else 1))      # (the last windows' replays have the threads to themselves)
                    nsub = max(1, min(split, nthreads, res.nbursts // 8))
                    cuts = [int(res.bursts[(res.nbursts * j) // nsub]["zone_first"]) for j in range(1, nsub)]
                    first = 0 if lo == 0 else int(res.bursts[0]["zone_first"])
                    starts, stops = [first] + cuts, cuts + [bound]
                    keep = [j for j in range(nsub) if stops[j] is None or stops[j] > starts[j]]
                    if sink:
                        safes = [int(res.bursts[(res.nbursts * j) // nsub]["safe_last"]) for j in range(nsub)]
                        out = [pool.submit(journal_window, k, res, piece, lo, [starts[j] for j in keep], [stops[j] for j in keep], [safes[j] for j in keep])]
                        busy[k % depth] = _All(out + [consumed[k]])
                    else:
                        out = [pool.submit(replay_window, k, res, piece, lo, [starts[j] for j in keep], [stops[j] for j in keep])]
                        busy[k % depth] = _All(out)
                elif sink:
                    out = [journal_window(k, res, piece, lo, [0 if lo == 0 else int(res.bursts[0]["zone_first"])], [bound], [int(res.bursts[0]["safe_last"])])]
                    busy[k % depth] = consumed[k]
                else:
                    out = [replay(k, res, piece, lo, bound)]
        finally:
            marks_seen[k].set()
            ctx_free[k % nctx].release()
        return out

    prod = threading.Thread(target=producer, name="rt-ingest-producer")
    import sys
    switch = sys.getswitchinterval()
    import gc
    gc_was = gc.isenabled()
    if not os.environ.get("RT_INGEST_GC"):
        gc.disable()                                      # a full collection walks every object of the process (PyTorch is loaded: tens of ms) with the interpreter lock held - every stage stalls at once
    sys.setswitchinterval(float(os.environ.get("RT_INGEST_SWITCH", "0.0002")))      # a dozen threads hand the interpreter lock around between system calls: at the default 5 ms a stage waits longer for the lock than it works
    try:
        import contextlib
        with (contextlib.nullcontext() if sink else open(tap_path, "wb")) as tapf:      # (the windowed decode's files are the finisher's)
            # software pipeline: the producer thread reads window after window and queues each one's copy and scan on the device; the fetchers bring
            # the windows' results to the host and hand them to the replay threads; this thread collects the pieces in window order
            if sink:                                          # (on this thread, which makes all its calls; the `finally` below ends it if anything fails)
                finisher = sink.finisher(hdr, cfg, full, opts, began)
                stats.update(bursts=0, fragment_work={k: 0 for k in pipeline.WORK_COUNTERS})
            prod.start()
            while True:
                k, fut = launched.get()
                if k is None:
                    if isinstance(fut, BaseException):
                        raise fut
                    break
                if fut is not None and finisher:
                    # the windowed decode: this thread is the finisher's - a window's journals are taken as soon as every window in front has been
                    for pc in fut.result():
                        got = pc.result() if hasattr(pc, "result") else pc
                        for j, jr in enumerate(got["journals"]):
                            live.discard(jr)
                            if finisher.limited:
                                finisher.discard(jr)
                                continue
                            if (got["lo"] > 0 or j > 0) and finisher.overrun(got["lo"] + got["safes"][j]):
                                # the block in front ended inside this fragment's first zone, past the proven restart: again, from there (pipeline.Finisher.overrun)
                                finisher.discard(jr)
                                jr = finisher.journal(first=False)
                                got["secs"][j] += pipeline.journal_fragments(hdr, cfg, fe_exact, got["res"], got["piece"], got["lo"], [finisher.final_row - got["lo"]],
                                                                             [got["stops"][j]], [jr], full, opts, exact_lock=exact_lock)[0]
                                stats["fragments_redone"] = stats.get("fragments_redone", 0) + 1
                            t_replay += got["secs"][j]
                            work = finisher.finish(jr)[2]
                            for key in work:
                                stats["fragment_work"][key] += work[key]
                            stats["fragments"] = stats.get("fragments", 0) + 1
                        stats["bursts"] += got["res"].nbursts
                        consumed[got["k"]].ev.set()
                    if finisher.limited:
                        stop.set()                                # (the block limit is reached: nothing more is read)
                        for ev in consumed:
                            ev.ev.set()
                elif fut is not None:
                    pieces.extend(fut.result())
            if finisher:
                f2, finisher = finisher, None
                fst = f2.end()
                total = int(fst["data_bytes"])
                stats.update(fst)
            for pc in pieces:                                 # in window order
                got = pc.result() if hasattr(pc, "result") else [pc]
                for data, st, secs in got:
                    t_replay += secs
                    tapf.write(data)
                    total += len(data)
                    for key in ("blocks", "tapemarks", "events_delivered", "exact_scans"):
                        stats[key] += int(st[key])
                    stats["all_ok"] = bool(stats["all_ok"] and st["all_ok"])      # (every fragment's blocks were clean: the reference's "ok")
            if total > 0 and not sink:
                tapf.write(b"\xff\xff\xff\xff")                   # src/readtape.c:1885
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t_start
    finally:                                              # (also when a replay raised: no thread, file or device context is left behind)
        sys.setswitchinterval(switch)
        if gc_was:
            gc.enable()
        stop.set()
        for ev in consumed or ():                         # (... or for a window the finisher will not take any more)
            ev.ev.set()
        for sem in ctx_free:                              # (a producer waiting for a context wakes up and sees the stop flag)
            sem.release()
        if prod.is_alive():
            prod.join()
        fetchers.shutdown(wait=True)
        if readers:
            readers.shutdown(wait=True)
        os.close(fd)
        if pool:
            pool.shutdown(wait=True, cancel_futures=True)
        if finisher is not None:                          # (a run that ended early; no fragment is running any more: the files are closed, the requests taken back)
            finisher.abandon()
        for jr in live:                                   # (journals of windows nobody collected)
            pipeline._load_decode_lib().rt_journal_free(jr)
        torch.cuda.synchronize(dev)
        fe_exact.close()
        for f in list(fes) + retired:
            f.close()
    if sink:
        stats["finisher_wait_seconds"] = fin_wait[0]
    if trace is not None:
        for k in range(len(spans)):                       # the device's own clock: a window's copy and the end of its scan, ms behind the start of the timed region
            if ("copy0", k) in gpu_ev:
                c0, c1, s1 = (gpu_ev["base"].elapsed_time(gpu_ev[(n, k)]) for n in ("copy0", "copy1", "scan1"))
                trace.append(("gpu_copy", k, c0 / 1e3, c1 / 1e3)); trace.append(("gpu_scan_done", k, c1 / 1e3, s1 / 1e3))
        stats["trace"] = sorted(trace, key=lambda x: x[2])
    stats.update(setup_seconds=t_start - t_enter, rows=data_end[0], seconds=dt, msamples_per_s=data_end[0] / dt / 1e6, replay_seconds=t_replay, read_seconds=t_read[0], scan_wait_seconds=wait_s[0],
                 replay_events_per_s=(stats["events_delivered"] / t_replay) if t_replay > 0 else None, tap_bytes=(total + (4 if total else 0)) if not sink else None, screen_floor_height=floor_state["floor"],
                 raw_rows=skip + data_end[0] * nth, bpi=cfg.bpi, skew=list(cfg.skew) if cfg.skew is not None else None)
    return stats


def decode_file_windows(path, out_base=None, tap_path=None, log_path=None, tap_format=True, labels=False, blklimit=None, textfile=None, created=None,
                        peakstats=False, quiet=False, hdr_overrides=None, in_name=None, parms_text=None, window_rows=1 << 24, halo_rows=1 << 17,
                        opts: pipeline.DecodeOptions | None = None, cfgkw=None, device="cuda:0", replay_threads: int = 1, read_threads: int = 4, replay_split: int = 1,
                        scan_contexts: int = 3, ramp: bool = True, subsample: int = 1, skip: int = 0, deskew: bool = False, skew=None, prepass_rows: int = 1 << 22):
    """decode_file_streaming's pipeline with the resident decode's outputs (pipeline.decode_tape's): the .tbin file `path` goes through the same reads, pinned
    buffers, streams, scan contexts, windows, halos and replay threads (window_rows ... prepass_rows: as there), but the windows' fragments write no pieces of a
    .tap - each journals its blocks (pipeline.journal_fragments) - and ONE finisher, on the caller's thread, takes a window's journals as soon as every window in
    front of it is done and puts the blocks out in tape order: out_base's files by the reference's names (<out_base>.tap, or with tap_format=False the numbered
    and label-named .bin files) or the one file tap_path, the log with its per-block lines and its summary (log_path; in_name, default `path`), the text file
    (textfile, created), labels, blklimit, peakstats / quiet exactly as decode_tape's arguments of those names.  With blklimit reached nothing more is read.
    hdr_overrides: what the command line sets over the header before anything is planned - order (or trkorder), bpi, ips, mode, ntrks; parms_text: a .parms text.
    The pre-passes (density, deskew) begin the log, and with peakstats the deskew pre-pass writes <base>.peakstats_deskew.csv, as in the resident decode.
    Returns decode_file_streaming's statistics with the resident decode's (blocks, tapemarks, data_bytes, all_ok ..., peakstats / skew_ok) in place of the sums,
    and bursts (the windows' own, summed), fragment_work (the fragments' replay counters, summed: what attempts, exact_scans ... are made of), windows_read, fragments, finisher_seconds (the finisher's own time) and finisher_wait_seconds (what the pipeline waited for it to release a window)."""
    lib = pipeline._load_decode_lib()
    if out_base is None and tap_path is None:
        raise ValueError("decode_file_windows: give out_base or tap_path")
    out = dict(tap_path=tap_path, log_path=log_path, out_base=out_base, in_name=(in_name or path) if out_base else None, tap_format=tap_format, labels=labels,
               blklimit=blklimit, textfile=textfile, created=created, quiet=quiet)
    out["peak_base"] = pipeline._request_peakstats(lib, peakstats, out_base, tap_path, quiet, bool(deskew) or skew is not None)
    try:
        return _decode_file(path, tap_path or out_base + ".tap", window_rows, halo_rows, opts, cfgkw, device, replay_threads, read_threads, replay_split, scan_contexts,
                            ramp, subsample, skip, deskew, skew, prepass_rows, _Windows(out, hdr_overrides, parms_text))
    finally:
        lib.rt_replay_set_peakstats(None, 0, 0)
