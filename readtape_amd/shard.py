"""Time sharding of one tape across the GPUs of a node.

The sample timeline is cut into contiguous row ranges, one per rank.  Bursts are independent (each
starts from reset state inside a dead-quiet zone), so the only coupling is at the seams: the burst that
straddles a seam is finished by the LEFT rank, which therefore needs the first rows of the right
rank's range — one neighbour halo (isend/irecv over RCCL/xGMI, or gloo on CPU), no collective on the
data path.  `rtfe_scan(..., own_rows)` then decodes exactly the bursts whose zone ends in the owned rows.
"""
from __future__ import annotations

import numpy as np

I64MAX = (1 << 63) - 1


def plan_shards(nrows: int, world: int, align: int = 1024):
    """[start, end) per rank.  Starts are multiples of `align` rows (a multiple of 64): 16-byte aligned for every track count, and
    on the 64-row grid of the quiet map, so a sharded scan finds exactly the zones of the whole-tape scan.  A tape too short to
    give every rank rows leaves the last ranks empty: (n, n)."""
    assert align % 64 == 0
    cuts = [min(nrows, (nrows * r // world) // align * align) for r in range(world)] + [nrows]
    for r in range(1, world):                       # (monotone; a rank whose slice would be empty gets (nrows, nrows) at the end)
        cuts[r] = max(cuts[r], cuts[r - 1])
    spans = [(cuts[r], cuts[r + 1]) for r in range(world)]
    live = [sp for sp in spans if sp[1] > sp[0]]
    return live + [(nrows, nrows)] * (world - len(live))


def plan_file_shards(raw_rows: int, world: int, subsample: int = 1, skip: int = 0, align: int = 1024):
    """The ranks' shares of a payload of `raw_rows` rows -> [(lo, hi, raw_lo, raw_hi)], one per rank: ingest.plan_windows' counterpart.
    Shards are planned in USED rows - of every `subsample` raw rows behind the first `skip`, the last (src/readtape.c:1407-1424, 1634-1641) - by
    plan_shards, so the cuts stay on the grid the ownership rule stands on.  Rank r owns the used rows [lo, hi) and reads the raw rows
    [raw_lo, raw_hi) = [skip + lo * n, skip + hi * n): its own share, no halo (the halo is exchanged in used rows).  An incomplete group of raw rows
    at the end of the payload is nobody's row; a tape too short for `world` ranks leaves the last ranks (n, n, ...)."""
    n, skip = int(subsample), int(skip)
    if n < 1 or skip < 0:
        raise ValueError(f"subsample {subsample} (at least 1), skip {skip} (not negative)")
    used = max(0, int(raw_rows) - skip) // n
    return [(lo, hi, skip + lo * n, skip + hi * n) for lo, hi in plan_shards(used, world, align)]


class ShardRows:
    """This rank's rows with room for the halo behind them: ONE buffer [n + halo_cap, ntrks], allocated once (the halo exchange
    receives straight into its tail; no concatenation per step)."""

    def __init__(self, own, halo_cap: int):
        import torch
        self.n = int(own.shape[0])
        self.cap = int(halo_cap)
        self.buf = torch.empty((self.n + self.cap, own.shape[1]), dtype=own.dtype, device=own.device)
        self.buf[: self.n].copy_(own)
        self.got = 0                                   # halo rows the last exchange delivered

    @classmethod
    def around(cls, buf, n: int):
        """Built around a buffer that already holds the own rows in buf[:n] (decode_file_sharded thins a rank's raw share straight into it): what
        lies behind them is the room for the halo.  Nothing is copied."""
        sr = cls.__new__(cls)
        sr.n, sr.buf, sr.got = int(n), buf, 0
        sr.cap = int(buf.shape[0]) - sr.n
        assert sr.cap >= 0
        return sr

    def own(self):
        return self.buf[: self.n]

    def rows(self):
        return self.buf[: self.n + self.got]

    def reserve(self, halo_cap: int):
        """A longer halo (the rare retry of decode_sharded): a new buffer, the own rows copied over once."""
        import torch
        if halo_cap > self.cap:
            nb = torch.empty((self.n + int(halo_cap), self.buf.shape[1]), dtype=self.buf.dtype, device=self.buf.device)
            nb[: self.n].copy_(self.buf[: self.n])
            self.buf, self.cap = nb, int(halo_cap)


def gather_lens(n: int, device, world: int, dist):
    """Every rank's row count, as a tensor all-gather (8 bytes per rank)."""
    import torch
    t = torch.tensor([int(n)], dtype=torch.int64, device=device)
    out = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(out, t)
    return [int(x.item()) for x in out]


def halo_plan(lens, halo_rows: int):
    """Who sends what to whom: rank d's halo is the tape rows [hi_d, hi_d + halo_rows) (cut at the tape's end), which may span several
    of the ranks behind it (a short shard, a long halo).  Returns [(src, dst, first row in src's range, rows, offset in dst's halo)]."""
    starts = [0]
    for n in lens:
        starts.append(starts[-1] + int(n))
    total = starts[-1]
    plan = []
    for d in range(len(lens) - 1):
        if lens[d] == 0:
            continue
        a, b = starts[d + 1], min(total, starts[d + 1] + int(halo_rows))
        for s in range(d + 1, len(lens)):
            lo, hi = max(a, starts[s]), min(b, starts[s + 1])
            if hi > lo:
                plan.append((s, d, lo - starts[s], hi - lo, lo - a))
    return plan


def exchange_halo(sr, halo_rows: int, rank: int, world: int, dist, lens=None):
    """sr: this rank's ShardRows (or a [n, ntrks] tensor: a ShardRows is made for it).  Fills the halo - the first rows of the ranks
    behind this one, as many of them as halo_rows reaches - by neighbour isend/irecv (RCCL over xGMI, or gloo), no collective on the
    data path; `lens` (every rank's row count) saves the 8-byte all-gather when the caller knows it.  Returns (rows_with_halo, own_rows)."""
    if not isinstance(sr, ShardRows):
        sr = ShardRows(sr, halo_rows if rank < world - 1 else 0)
    if world == 1:
        sr.got = 0
        return sr.rows(), sr.n
    if lens is None:
        lens = gather_lens(sr.n, sr.buf.device, world, dist)
    plan = halo_plan(lens, halo_rows)
    sr.reserve(max([off + cnt for _, d, _, cnt, off in plan if d == rank], default=0))      # (what the plan delivers: the tape's end cuts the last halos short - ADVICE r3)
    ops, got = [], 0
    for s, d, first, cnt, off in plan:
        if s == rank:
            ops.append(dist.P2POp(dist.isend, sr.buf[first: first + cnt], d))
        elif d == rank:
            ops.append(dist.P2POp(dist.irecv, sr.buf[sr.n + off: sr.n + off + cnt], s))
            got = max(got, off + cnt)
    if ops:
        for w in dist.batch_isend_irecv(ops):
            w.wait()
    sr.got = got
    return sr.rows(), sr.n


def absolute_bursts(res, start_row: int):
    """Burst table of one rank with row fields shifted to tape-absolute rows."""
    b = res.bursts.copy()
    for f in ("zone_first", "zone_end", "reset_sample", "safe_last", "end_sample"):
        m = b[f] >= 0
        b[f][m] += start_row
    return b


def flatten_events(res, bursts_abs, parmset: int):
    """[(absolute detection row, trk, kind, v_peak bits, agc bits, left_distance, adj)] over all bursts of one rank."""
    out = []
    for i in range(res.nbursts):
        ev = res.events(i, parmset)
        n0 = bursts_abs[i]["reset_sample"] + ev["sample"].astype(np.int64)
        out.append(np.stack([n0, ev["trk"].astype(np.int64), ev["flags"].astype(np.int64), ev["v_peak"].view("u4").astype(np.int64),
                             ev["agc_gain"].view("u4").astype(np.int64), ev["left_distance"].astype(np.int64)], 1))
    return np.concatenate(out) if out else np.zeros((0, 6), np.int64)


def _agree(who, more, err, rank, world, dist, dev, cleanup=None, reraise=False):
    """[someone needs a longer halo, someone failed, who] - one 24-byte all-reduce, every rank in the same place.  A failure on one rank stops every
    rank before the next collective: the failing rank raises its error (as it is with reraise, else wrapped with its rank), the others a RuntimeError
    that names the first rank that failed.  Returns whether someone needs more."""
    import torch
    t = torch.tensor([1 if more else 0, 1 if err is not None else 0, world - rank if err is not None else 0], dtype=torch.int64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    v = [int(x) for x in t.tolist()]
    if v[1]:
        if cleanup:
            cleanup()
        if err is not None:
            if reraise:
                raise err
            raise RuntimeError(f"{who}: rank {rank} failed: {err!r}") from err
        raise RuntimeError(f"{who}: another rank failed (rank {world - v[2]}); this rank stops with it")
    return bool(v[0])


_SETTLED_WORDS = 3 + 19                                   # status, the density's bits, whether delays exist, the delays (MAXTRKS of them)


def _settle_on_rank0(settle, hdr, cfgkw, rank, dist, dev):
    """The pre-passes' result from rank 0 to every rank: rank 0 runs `settle()` -> cfgkw with "bpi" / "skew"; the others launch nothing and read nothing.
    One small int64 tensor is broadcast: status, the density (a double's bits), whether delays exist, the delays.  -> (cfgkw, rank 0's error on rank 0):
    the caller agrees on the failure (_agree) before the next collective."""
    import struct
    import torch
    err, words = None, [0] * _SETTLED_WORDS
    if rank == 0:
        try:
            cfgkw = settle()
            skew = cfgkw.get("skew")
            words[1] = struct.unpack("<q", struct.pack("<d", float(cfgkw.get("bpi") or 0.0)))[0]
            if skew is not None:
                words[2] = 1
                words[3: 3 + len(skew)] = [int(x) for x in skew]
        except Exception as e:                                # (agreed on below)
            err, words[0] = e, 1
    t = torch.tensor(words, dtype=torch.int64, device=dev)
    dist.broadcast(t, src=0)
    v = [int(x) for x in t.tolist()]
    if rank != 0 and not v[0]:
        cfgkw = dict(cfgkw)
        bpi = struct.unpack("<d", struct.pack("<q", v[1]))[0]
        if bpi > 0:
            cfgkw["bpi"] = bpi
        if v[2]:
            cfgkw["skew"] = v[3: 3 + hdr.ntrks]
    return cfgkw, err


def _decode_shards(who, hdr, sr, lo, n_total, lens, rank, world, dist, tap_path, opts, full, cfgkw, make_fe, host_rows, halo_rows):
    """What decode_sharded and decode_file_sharded share: this rank's own rows are sr.own() = the tape's rows [lo, lo + sr.n), `lens` every rank's count.
    -> (the per-rank records, the front end's configuration)."""
    import torch
    from . import frontend, pipeline
    cfg = frontend.FrontEndConfig.from_header(hdr, parmsets=pipeline.frontend_parmsets(full), **cfgkw)
    fe = make_fe(cfg)
    n = sr.n
    dev = sr.buf.device
    is_last = lo + n >= n_total
    halo = int(halo_rows)
    err = None

    def agree(more):
        return _agree(who, more, err, rank, world, dist, dev, cleanup=fe.close)

    res, nb, bound, piece = None, 0, None, None
    while True:
        with_halo, own_rows = exchange_halo(sr, halo, rank, world, dist, lens=lens)
        more = False
        try:
            piece = with_halo.numpy() if host_rows else with_halo
            res, nb, bound = pipeline.scan_fragment(fe, piece, own_rows, lo, lo == 0, is_last)() if n > 0 else (None, 0, None)
            got_all = lo + int(piece.shape[0]) >= n_total
            more = n > 0 and nb is None and not got_all
        except Exception as e:                                # (agreed on below: no rank is left in a collective)
            err = e
        if not agree(more):
            break
        halo = min(halo * 4, n_total)                         # (a halo as long as the tape reaches its end from anywhere)
    tap_bytes = b""
    stats = dict(blocks=0, tapemarks=0, events_delivered=0)
    try:
        if n > 0 and res.nbursts > 0:
            import os, tempfile
            with tempfile.TemporaryDirectory() as wd:
                frag = os.path.join(wd, f"r{rank}.tap")
                start = 0 if lo == 0 else int(res.bursts[0]["zone_first"])
                stats = pipeline.decode_fragment(hdr, cfg, fe, res, piece, lo, start, bound, frag, full, opts, make_fe)
                tap_bytes = open(frag, "rb").read()
    except Exception as e:
        err = e
    agree(False)
    # the per-rank records: int64 tensors, all-gathered
    ev = [int(x) for x in res.counts.sum(axis=(0, 2))] if n > 0 and res.nbursts else [0] * len(full)
    mine = torch.tensor([rank, lo, lo + n, int(res.nbursts) if n > 0 else 0, int(stats["blocks"]), int(stats["tapemarks"]), len(tap_bytes)] + ev,
                        dtype=torch.int64, device=dev)
    recs = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(recs, mine)
    table, off = [], 0
    for t in recs:
        v = [int(x) for x in t.tolist()]
        table.append(dict(rank=v[0], lo=v[1], hi=v[2], bursts=v[3], blocks=v[4], tapemarks=v[5], tap_len=v[6], events=v[7:], tap_offset=off))
        off += v[6]
    # the .tap pieces: uint8 tensors padded to the longest piece, gathered on rank 0
    longest = max(1, max(r["tap_len"] for r in table))
    mine_b = torch.zeros(longest, dtype=torch.uint8, device=dev)
    if tap_bytes:
        mine_b[: len(tap_bytes)] = torch.frombuffer(bytearray(tap_bytes), dtype=torch.uint8).to(dev)
    pieces = [torch.zeros_like(mine_b) for _ in range(world)] if rank == 0 else None
    dist.gather(mine_b, pieces, dst=0)
    if rank == 0 and tap_path:
        with open(tap_path, "wb") as f:
            for r, pc in zip(table, pieces):
                f.write(pc[: r["tap_len"]].cpu().numpy().tobytes())
            if off > 0:
                f.write(b"\xff\xff\xff\xff")                # src/readtape.c:1885
    fe.close()
    return table, cfg


def decode_sharded(hdr, own, lo: int, n_total: int, rank: int, world: int, dist, tap_path: str | None, opts=None, fe_factory=None,
                   halo_rows: int = 1 << 16, cfgkw=None, deskew: bool = False, skew=None, peakstats: bool = False):
    """The whole multi-rank decode of ONE tape: `own` = this rank's rows [lo, lo + len(own)) of the n_total-row tape.
      1. halo exchange (isend/irecv; repeated with a four times longer halo - it may then span several of the ranks behind - while some
         rank's last own burst runs past it; the halo stops growing at the tape's end, so the loop ends),
      2. rtfe_scan of own + halo with the own_rows ownership rule,
      3. host replay of the own bursts -> this rank's piece of the .tap,
      4. tensor all-gather of one small record per rank {own range, bursts, events per parameter set, .tap bytes} (the only collectives),
      5. rank 0 gathers the pieces (uint8 tensors, padded to the longest) in rank order, concatenates them and ends the file.
    A failure on one rank (a fatal reference condition in its replay, a device error) is agreed on by all ranks before the next
    collective: every rank raises, none is left waiting.  Returns the list of per-rank records (every rank).
    A header without a density (NRZI), deskew=True without `skew` (the delays, in samples per track): rank 0 runs pipeline.detect_density /
    calibrate_deskew on ITS OWN rows and broadcasts what they find; where their stopping rule is not met inside rank 0's rows and other ranks hold
    more, every rank raises a RuntimeError (pass the values in cfgkw / skew, or start from the file: decode_file_sharded reads a longer prefix)."""
    from . import frontend, ingest, pipeline
    pipeline.refuse_peakstats(peakstats, "shard.decode_sharded")
    opts = opts or pipeline.DecodeOptions()
    full = pipeline.default_parmsets(hdr.mode, opts.nparmsets or (15 if opts.multiple_tries else 1))
    cfgkw = dict(cfgkw or {})
    if skew is not None:
        cfgkw["skew"] = [int(x) for x in skew]
    make_fe = fe_factory or frontend.FrontEnd
    n = int(own.shape[0])
    dev = own.device
    need_bpi, need_skew = ingest._prepass_needs(hdr, cfgkw, deskew)
    if need_bpi or need_skew:
        def run(what, fn):
            got = fn(own.numpy() if fe_factory is not None else own, lo + n < n_total) if n > 0 else None
            if got is None:
                raise RuntimeError(f"decode_sharded: {what} is undecided inside rank 0's {n} rows: pass the values (cfgkw bpi=, skew=) or use "
                                   "decode_file_sharded, which reads as long a prefix of the file as the pre-passes need")
            return got
        cfgkw, err = _settle_on_rank0(lambda: ingest._settle(hdr, full, opts, cfgkw, need_bpi, need_skew, make_fe, run), hdr, cfgkw, rank, dist, dev)
        _agree("decode_sharded", False, err, rank, world, dist, dev, reraise=True)
    lens = gather_lens(n, dev, world, dist)
    sr = ShardRows(own, min(halo_rows, max(0, n_total - lo - n)))
    return _decode_shards("decode_sharded", hdr, sr, lo, n_total, lens, rank, world, dist, tap_path, opts, full, cfgkw, make_fe,
                          fe_factory is not None, halo_rows)[0]


def _refusing_peakstats(fn):
    """fn with one keyword more, peakstats (False): True raises pipeline.refuse_peakstats' ValueError before anything is read or exchanged.  The function's
    own parameter list stays what its callers and tests/test_shard_file_plan.py know (inspect.signature follows __wrapped__)."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, peakstats: bool = False, **kw):
        from . import pipeline
        pipeline.refuse_peakstats(peakstats, "shard." + fn.__name__)
        return fn(*args, **kw)
    return wrapper


@_refusing_peakstats
def decode_file_sharded(path, tap_path, rank: int, world: int, dist, opts=None, cfgkw=None, halo_rows: int = 1 << 16, subsample: int = 1, skip: int = 0,
                        deskew: bool = False, skew=None, prepass_rows: int = 1 << 22, device="cuda:0", align: int = 1024, fe_factory=None,
                        _lib_path=None, _backend=None):
    """decode_sharded from the .tbin file `path` to the SIMH file `tap_path`, with the reader's options of ingest.decode_file_streaming (subsample, skip, a
    header without bpi, deskew / skew).  Every rank calls it; rank 0 writes tap_path (None is accepted on the others).
      1. plan_file_shards: the ranks' shares in used rows and the raw rows each is made of.
      2. Every rank reads ITS raw rows (rt_read_mt into a pinned buffer), uploads them and thins them on the device straight into the buffer its halo
         will be received into (rtfe_decimate_rows: with subsample 1 a copy; in the same pass the first raw row with the end marker).
      3. Rank 0 runs the pre-passes (ingest._prepasses: on a prefix it reads from the file itself, grown by their rule - it may reach past rank 0's
         share) and broadcasts the density and the delays in one small tensor; the other ranks launch and read nothing for them.
      4. One all-reduce MIN of lo + mark // subsample gives the data's end E: n_total = min(used rows, E); every rank clips its rows to it, a rank
         wholly behind it decodes nothing.  (A marker among the skipped rows is not looked at; a group the marker cuts short is dropped.)
      5. decode_sharded's halo exchange, scans, replays and gather on the thinned rows.
    Failures (PE without a density, an undecided prefix that does not fit, a short read, ...) are agreed on before the next collective: the failing rank
    raises its own error, the others a RuntimeError that names it.  Whirlwind files and bad options raise on every rank before any collective.
    fe_factory / _lib_path / _backend: hooks for tests/cpu_emul (with a backend of the caller's the rows are host tensors).
    Returns (the per-rank records, dict(bpi, skew, rows = used rows decoded, raw_rows = the payload rows they stand for, shards = the plan))."""
    import os
    import torch
    from . import frontend, ingest, pipeline, tbin
    opts = opts or pipeline.DecodeOptions()
    hdr, off, raw_rows = ingest._payload_geometry(path)
    if hdr.mode == tbin.MODE_WW:
        raise NotImplementedError("Whirlwind tapes are one chain (no independent fragments): read the file and use pipeline.decode_tape_ww")
    nth, skip = int(subsample), int(skip)
    if nth < 1 or skip < 0:
        raise ValueError(f"subsample {subsample} (at least 1), skip {skip} (not negative)")
    who = "decode_file_sharded"
    ntrks = hdr.ntrks
    plan = plan_file_shards(raw_rows, world, nth, skip, align)
    lo, hi, raw_lo, raw_hi = plan[rank]
    used = max(0, raw_rows - skip) // nth
    full = pipeline.default_parmsets(hdr.mode, opts.nparmsets or (15 if opts.multiple_tries else 1))
    cfgkw = dict(cfgkw or {})
    if skew is not None:
        cfgkw["skew"] = [int(x) for x in skew]
    on_host = _backend is not None
    dev = torch.device("cpu") if on_host else torch.device(device)
    make_fe = fe_factory or (lambda c: frontend.FrontEnd(c, device=device))
    view = (lambda t: t.numpy()) if on_host else (lambda t: t)
    err, mark, buf, fd = None, I64MAX, None, None
    try:
        # the own share: raw rows -> pinned -> device -> thinned into the head of the buffer the halo is received behind
        be, lib, dlib = _backend or frontend.TorchBackend(device), frontend._load_library(_lib_path), pipeline._load_decode_lib()
        fd = os.open(path, os.O_RDONLY)
        buf = torch.empty((hi - lo + min(int(halo_rows), max(0, used - hi)), ntrks), dtype=torch.int16, device=dev)
        if hi > lo:
            host = torch.empty((raw_hi - raw_lo, ntrks), dtype=torch.int16, pin_memory=not on_host)
            if dlib.rt_read_mt(fd, host.numpy().ctypes.data, off + raw_lo * 2 * ntrks, (raw_hi - raw_lo) * 2 * ntrks, 4) != 0:
                raise IOError("short read")
            d_raw = host if on_host else host.to(dev, non_blocking=True)
            d_mark = be.empty(16)
            frontend.decimate_rows(lib, be, view(d_raw), raw_hi - raw_lo, nth - 1, nth, view(buf[: hi - lo]), d_mark)
            mark = int(be.to_numpy(d_mark, np.int64)[0])      # (waits for the thinning: the raw staging buffer is free from here on)
            del d_raw, host
    except Exception as e:                                    # (agreed on below)
        err = e
    need_bpi, need_skew = ingest._prepass_needs(hdr, cfgkw, deskew)
    try:
        if (need_bpi or need_skew) and used > 0:
            def settle():
                if err is not None:                           # (rank 0's own share failed: the pre-passes are not run behind that)
                    raise err
                return ingest._prepasses(hdr, fd, off + skip * 2 * ntrks, used, nth, full, opts, cfgkw, deskew, int(prepass_rows), device,
                                         fe_factory=make_fe, backend=_backend, lib=lib)
            cfgkw, err0 = _settle_on_rank0(settle, hdr, cfgkw, rank, dist, dev)
            err = err or err0
    finally:
        if fd is not None:
            os.close(fd)
    _agree(who, False, err, rank, world, dist, dev, reraise=True)
    # the data's end: the first raw row at or behind `skip` with the marker, in used rows (a group it cuts short is dropped)
    t = torch.tensor([lo + mark // nth if mark != I64MAX else I64MAX], dtype=torch.int64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    n_total = min(used, int(t.item()))
    lens = [max(0, min(h, n_total) - l) for l, h, _, _ in plan]
    sr = ShardRows.around(buf, lens[rank])
    table, cfg = _decode_shards(who, hdr, sr, min(lo, n_total), n_total, lens, rank, world, dist, tap_path, opts, full, cfgkw, make_fe, on_host, halo_rows)
    return table, dict(bpi=cfg.bpi, skew=list(cfg.skew) if cfg.skew is not None else None, rows=n_total, raw_rows=skip + n_total * nth, shards=plan)
