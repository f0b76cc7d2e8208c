"""GPU: shard.decode_file_sharded - the multi-rank decode of one capture file with the reader's options (a header without a density, -deskew,
-subsample, -skip) - and shard.decode_sharded's deskew=, against the golden tapes' reference output, the resident decode and the streaming reader.
The ranks are threads of tests/local_group.py with the real FrontEnd: one process holds the GPU, and the halo-growing loop, the ownership rule, the
per-rank replay and the gather run as they would on N devices (RCCL and a second device are what this does not run)."""
import dataclasses
import threading

import numpy as np
import pytest

import local_group
from golden_util import load_case
from readtape_amd import ingest, pipeline, shard, synth, tbin

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _opts_of(g):
    """The golden's reference options as tests/test_gpu_ingest_options.py maps them."""
    o = g["oracle_opts"]
    return dict(opts=pipeline.DecodeOptions(multiple_tries="-m" in o, correct="-correct" in o), deskew="-deskew" in o,
                subsample=next((int(a[11:]) for a in o if a.startswith("-subsample=")), 1))


_cache = {}


def _resident(key, hdr, rows, tmp_path, **kw):
    """(.tap, stats) of pipeline.decode_tape - computed once per key, shared, left unchanged."""
    if key not in _cache:
        tap = str(tmp_path / "resident.tap")
        stats, _ = pipeline.decode_tape(hdr, rows, tap, **kw)
        _cache[key] = (open(tap, "rb").read(), stats)
    return _cache[key]


def _write(tmp_path, hdr, rows):
    """header + rows + one marker (not tbin.write_tbin: some of these payloads carry an end marker inside)"""
    path = str(tmp_path / "t.tbin")
    with open(path, "wb") as f:
        f.write(tbin.pack_header(hdr))
        f.write(np.ascontiguousarray(rows, dtype="<i2").tobytes())
        f.write(np.array([tbin.END_MARK], dtype="<i2").tobytes())
    return path


def _sharded(hdr, rows, tmp_path, world, **kw):
    """-> (.tap of rank 0, the ranks' table, info); every rank returned the same table and info"""
    path, tap = _write(tmp_path, hdr, rows), str(tmp_path / "sharded.tap")
    out = local_group.run(world, lambda rank, dist: shard.decode_file_sharded(path, tap if rank == 0 else None, rank, world, dist, **kw))
    assert all(o == out[0] for o in out)
    table, info = out[0]
    assert [t["rank"] for t in table] == list(range(world)) and info["shards"] == shard.plan_file_shards(rows.shape[0], world, kw.get("subsample", 1), kw.get("skip", 0))
    return open(tap, "rb").read(), table, info


@pytest.fixture(scope="module")
def oversampled():
    """tests/test_gpu_ingest_options.py's: a dozen NRZI blocks sampled every 320 ns, four times the usual rate; blocks up to 900 bytes - longer than
    the halos below, so halos have to grow."""
    spec = synth.TapeSpec(mode=tbin.MODE_NRZI, ntrks=9, bpi=800.0, ips=50.0, tdelta_ns=320, maxvolts=4.4, pulse_w=0.22, seed=83)
    rng = np.random.default_rng(83)
    items = [("block", p) for p in synth.random_payloads(rng, 12, 200, 900)]
    items.insert(5, ("mark",))
    return synth.make_tape(spec, items, gap_samples=12000)


def _count_prepasses(monkeypatch):
    """pipeline.detect_density / calibrate_deskew, counted: [(name, thread, rows they were given, whether they answered None)]"""
    calls = []
    for fn_name in ("calibrate_deskew", "detect_density"):
        def counted(*a, _fn=getattr(pipeline, fn_name), _name=fn_name, **kw):
            r = _fn(*a, **kw)
            calls.append((_name, threading.current_thread().name, int(a[1].shape[0]), r is None))
            return r
        monkeypatch.setattr(pipeline, fn_name, counted)
    return calls


# ---- the goldens ----

@pytest.mark.parametrize("name,world", [("nrzi9_nobpi", 3), ("nrzi9_deskew_long", 2), ("gcr_deskew", 2), ("nrzi9_nobpi_deskew", 3), ("nrzi9_sub2", 2)])
def test_goldens(name, world, tmp_path, gpu, monkeypatch):
    g = load_case(name)
    kw = _opts_of(g)
    _, want = _resident(name, g["hdr"], g["rows"], tmp_path, **kw)
    calls = _count_prepasses(monkeypatch)
    tap, table, info = _sharded(g["hdr"], g["rows"], tmp_path, world, halo_rows=1 << 12, **kw)
    assert tap == g["tap"]
    assert info["bpi"] == want["bpi"] > 0 and info["skew"] == want["skew"]
    assert info["rows"] == g["rows"].shape[0] // kw["subsample"] and info["raw_rows"] == info["rows"] * kw["subsample"]
    assert sum(t["bursts"] > 0 for t in table) >= 2, table
    assert {c[1] for c in calls} <= {"local-rank-0"} and bool(calls) == (kw["deskew"] or not g["hdr"].bpi > 0), calls


# ---- the pre-passes ----

def test_a_short_first_prefix_grows_past_rank_0s_share(tmp_path, gpu, monkeypatch):
    g = load_case("nrzi9_nobpi_deskew")
    _, want = _resident("nrzi9_nobpi_deskew", g["hdr"], g["rows"], tmp_path, **_opts_of(g))
    calls = _count_prepasses(monkeypatch)
    tap, table, info = _sharded(g["hdr"], g["rows"], tmp_path, 3, halo_rows=1 << 12, prepass_rows=4096, **_opts_of(g))
    assert tap == g["tap"] and info["bpi"] == want["bpi"] and info["skew"] == want["skew"]
    assert {c[0] for c in calls} == {"detect_density", "calibrate_deskew"} and {c[1] for c in calls} == {"local-rank-0"}, calls
    assert any(c[3] for c in calls) and calls[0][2] == 4096, calls                          # undecided at least once: the prefix grew
    assert max(c[2] for c in calls) > info["shards"][0][1], (calls, info["shards"])         # ... past what rank 0 owns


def test_given_delays_run_no_prepass(tmp_path, gpu, monkeypatch):
    g = load_case("nrzi9_deskew_long")
    _, want = _resident("nrzi9_deskew_long", g["hdr"], g["rows"], tmp_path, **_opts_of(g))

    def never(*a, **kw):
        raise AssertionError("a pre-pass ran")
    monkeypatch.setattr(pipeline, "calibrate_deskew", never)
    monkeypatch.setattr(pipeline, "detect_density", never)
    monkeypatch.setattr(shard, "_settle_on_rank0", never)                                   # (nothing is broadcast either)
    tap, _, info = _sharded(g["hdr"], g["rows"], tmp_path, 2, halo_rows=1 << 12, deskew=True, skew=want["skew"])
    assert tap == g["tap"] and info["skew"] == want["skew"]


# ---- -subsample ----

def _watch_halos(monkeypatch):
    asked = []

    def watched(sr, halo_rows, *a, _fn=shard.exchange_halo, **kw):
        asked.append(int(halo_rows))
        return _fn(sr, halo_rows, *a, **kw)
    monkeypatch.setattr(shard, "exchange_halo", watched)
    return asked


@pytest.mark.parametrize("n", [2, 3])
def test_subsample_equals_the_resident_decode(n, oversampled, tmp_path, gpu, monkeypatch):
    hdr = dataclasses.replace(oversampled.spec.header(), tdelta_ns=320 * n)      # (the header's tdelta is the time between USED rows)
    want, stats = _resident(("whole", n), hdr, oversampled.rows, tmp_path, subsample=n)
    assert stats["blocks"] == 12 and stats["tapemarks"] == 1
    asked = _watch_halos(monkeypatch)
    tap, table, info = _sharded(hdr, oversampled.rows, tmp_path, 3, subsample=n, halo_rows=1 << 12)
    assert tap == want
    assert info["rows"] == oversampled.rows.shape[0] // n and info["raw_rows"] == info["rows"] * n
    assert sum(t["blocks"] for t in table) == 12 and all(t["bursts"] > 0 for t in table)
    assert max(asked) > (1 << 12), asked                    # a halo had to grow


@pytest.mark.parametrize("where", ["rank1_skipped", "rank1_kept", "rank0_halo", "rank2"])
def test_an_end_marker_inside_the_payload(where, oversampled, tmp_path, gpu):
    """The data end at the first RAW row whose head-0 sample is the marker, whichever place in its group it has (src/readtape.c:1407-1413): one all-reduce
    turns the one rank's find into every rank's n_total."""
    n, world = 2, 3
    hdr = dataclasses.replace(oversampled.spec.header(), tdelta_ns=320 * n)
    (_, _, _, _), (lo1, hi1, _, _), (lo2, hi2, _, _) = shard.plan_file_shards(oversampled.rows.shape[0], world, n)
    used, kept = {"rank1_skipped": (lo1 + (hi1 - lo1) * 5 // 8, 0), "rank1_kept": (lo1 + (hi1 - lo1) * 5 // 8, 1), "rank0_halo": (lo1 + 700, 0),
                  "rank2": (lo2 + 4090, 1)}[where]
    m = used * n + (n - 1 if kept else 0)                   # (of every n raw rows the last is the used one)
    rows = oversampled.rows.copy()
    rows[m, 0] = tbin.END_MARK
    want, _ = _resident(("cut", m), hdr, oversampled.rows[:m], tmp_path, subsample=n)
    tap, table, info = _sharded(hdr, rows, tmp_path, world, subsample=n, halo_rows=1 << 12)
    assert info["rows"] == m // n == used and info["raw_rows"] == used * n
    assert tap == want and len(want) > 1000
    for t, (lo, hi, _, _) in zip(table, info["shards"]):
        assert (t["lo"], t["hi"]) == (min(lo, used), min(hi, used))
        if lo >= used:                                      # wholly behind the marker
            assert t["bursts"] == 0 and t["tap_len"] == 0, table
    assert (table[2]["hi"] == table[2]["lo"]) == (where != "rank2")


# ---- -skip ----

def test_skip(tmp_path, gpu):
    """-skip: the decode of rows[skip:] - a skip that is a multiple of neither 1024 nor the subsampling step, and a marker among the skipped rows is not looked at."""
    tape = synth.nrzi_tape(seed=84, nblocks=20, minlen=200, maxlen=900, marks_every=6, gap_samples=3000)
    hdr, skip = tape.spec.header(), 1531
    want, _ = _resident("skip", hdr, tape.rows[skip:], tmp_path)
    rows = tape.rows.copy()
    rows[777, 0] = tbin.END_MARK
    tap, table, info = _sharded(hdr, rows, tmp_path, 2, skip=skip, halo_rows=1 << 12)
    assert tap == want and len(tap) > 1000
    assert info["rows"] == tape.rows.shape[0] - skip and info["raw_rows"] == tape.rows.shape[0] and all(t["bursts"] > 0 for t in table)


# ---- one rank: the streaming reader's answers ----

@pytest.mark.parametrize("which", ["nrzi9_nobpi_deskew", "oversampled"])
def test_world_1_equals_the_streaming_reader(which, oversampled, tmp_path, gpu):
    if which == "oversampled":
        hdr, rows, kw = dataclasses.replace(oversampled.spec.header(), tdelta_ns=640), oversampled.rows, dict(subsample=2)
    else:
        g = load_case(which)
        hdr, rows, kw = g["hdr"], g["rows"], _opts_of(g)
    tap, table, info = _sharded(hdr, rows, tmp_path, 1, halo_rows=1 << 12, **kw)
    stap = str(tmp_path / "streamed.tap")
    st = ingest.decode_file_streaming(_write(tmp_path, hdr, rows), stap, window_rows=1 << 15, halo_rows=1 << 12, **kw)
    assert tap == open(stap, "rb").read() and len(tap) > 1000
    assert {k: info[k] for k in ("bpi", "skew", "rows", "raw_rows")} == {k: st[k] for k in ("bpi", "skew", "rows", "raw_rows")}
    assert table[0]["blocks"] == st["blocks"] and table[0]["tapemarks"] == st["tapemarks"]


# ---- refusals ----

def test_a_pe_header_without_density_stops_every_rank(tmp_path, gpu):
    tape = synth.pe_tape(seed=5, nblocks=2)
    path = _write(tmp_path, dataclasses.replace(tape.spec.header(), bpi=0.0), tape.rows)
    out = local_group.run(2, lambda rank, dist: shard.decode_file_sharded(path, None, rank, 2, dist), raise_first=False)
    assert isinstance(out[0], NotImplementedError) and "NRZI only" in str(out[0])
    assert type(out[1]) is RuntimeError and "another rank failed (rank 0)" in str(out[1])      # (its own error: not the group's, not a timeout)


def test_a_whirlwind_file_and_bad_options_are_refused_before_any_collective(tmp_path, gpu):
    g = load_case("ww")
    with pytest.raises(NotImplementedError, match="Whirlwind"):
        shard.decode_file_sharded(_write(tmp_path, g["hdr"], g["rows"]), None, 0, 2, None)      # (no group: a collective would raise something else)
    g = load_case("nrzi9_sub2")
    for bad in (dict(subsample=0), dict(skip=-1)):
        with pytest.raises(ValueError):
            shard.decode_file_sharded(_write(tmp_path, g["hdr"], g["rows"]), None, 1, 2, None, **bad)


# ---- the resident entry point ----

def _resident_sharded(hdr, rows, cut, tmp_path, torch, **kw):
    n = rows.shape[0]
    spans, tap = [(0, cut), (cut, n)], str(tmp_path / "resident_sharded.tap")

    def rank_fn(rank, dist):
        lo, hi = spans[rank]
        own = torch.from_numpy(np.ascontiguousarray(rows[lo:hi])).cuda()
        return shard.decode_sharded(hdr, own, lo, n, rank, 2, dist, tap if rank == 0 else None, halo_rows=1 << 12, **kw)
    return tap, rank_fn


def _watch_broadcast(monkeypatch):
    """what shard._settle_on_rank0 hands each rank: {thread: cfgkw}"""
    seen = {}

    def watched(*a, _fn=shard._settle_on_rank0, **kw):
        r = _fn(*a, **kw)
        seen[threading.current_thread().name] = r[0]
        return r
    monkeypatch.setattr(shard, "_settle_on_rank0", watched)
    return seen


def test_resident_shards_calibrate_on_rank_0_and_broadcast(tmp_path, gpu, monkeypatch):
    """A dozen skewed NRZI blocks of 200 - 900 bytes: the calibration's stopping rule (1000 transitions on every track) is met inside rank 0's half, so
    rank 0 decides alone and rank 1 - which owns six of the blocks - scans with the delays it was sent."""
    tape = synth.nrzi_tape(seed=85, nblocks=12, minlen=200, maxlen=900, marks_every=6, gap_samples=3000, skew_cells=(0.0, 0.12, 0.05, 0.18, 0.02, 0.15, 0.08, 0.03, 0.10))
    hdr = tape.spec.header()
    want, stats = _resident("skewed", hdr, tape.rows, tmp_path, deskew=True)
    assert stats["blocks"] == 12 and max(stats["skew"]) >= 3
    calls, seen = _count_prepasses(monkeypatch), _watch_broadcast(monkeypatch)
    tap, rank_fn = _resident_sharded(hdr, tape.rows, shard.plan_shards(tape.rows.shape[0], 2)[0][1], tmp_path, gpu, deskew=True)
    out = local_group.run(2, rank_fn)
    assert open(tap, "rb").read() == want and out[0] == out[1] and all(t["blocks"] >= 5 for t in out[0])
    assert [c[:2] for c in calls] == [("calibrate_deskew", "local-rank-0")], calls
    assert {k: v["skew"] for k, v in seen.items()} == {"local-rank-0": stats["skew"], "local-rank-1": stats["skew"]}


def test_resident_shards_detect_the_density_on_rank_0_and_broadcast(tmp_path, gpu, monkeypatch):
    """nrzi9_nobpi: the 9999 transitions of the density detection lie inside the first 58368 rows, so with a cut at 61440 rank 0 decides alone."""
    g = load_case("nrzi9_nobpi")
    _, want = _resident("nrzi9_nobpi", g["hdr"], g["rows"], tmp_path, **_opts_of(g))
    calls, seen = _count_prepasses(monkeypatch), _watch_broadcast(monkeypatch)
    tap, rank_fn = _resident_sharded(g["hdr"], g["rows"], 61440, tmp_path, gpu)
    out = local_group.run(2, rank_fn)
    assert open(tap, "rb").read() == g["tap"] and out[0] == out[1] and all(t["bursts"] > 0 for t in out[0])
    assert [c[:2] for c in calls] == [("detect_density", "local-rank-0")], calls
    assert {k: v["bpi"] for k, v in seen.items()} == {"local-rank-0": want["bpi"], "local-rank-1": want["bpi"]} and want["bpi"] > 0


def test_resident_shards_of_nrzi9_deskew_long(tmp_path, gpu, monkeypatch):
    """nrzi9_deskew_long with deskew=True on two ranks gives the reference's .tap.  On this tape (and on every -deskew golden) the calibration's stopping
    rule is met only in the tape's last block - a prefix of 66560 of its 67141 rows is still undecided -, and rows behind rank 0's are `more_rows`: so rank 0
    can decide only where it owns the whole tape, and rank 1 is the empty last rank of a tape too short for two (plan_shards' (n, n)): it takes part in the
    broadcast and in every collective and decodes nothing.  Any other cut is the refusal of the next test."""
    g = load_case("nrzi9_deskew_long")
    kw = _opts_of(g)
    assert kw.pop("subsample") == 1 and kw["deskew"]
    calls = _count_prepasses(monkeypatch)
    tap, rank_fn = _resident_sharded(g["hdr"], g["rows"], g["rows"].shape[0], tmp_path, gpu, **kw)
    out = local_group.run(2, rank_fn)
    assert open(tap, "rb").read() == g["tap"] and out[0] == out[1] and out[0][1]["bursts"] == 0 and out[0][0]["bursts"] > 0
    assert [c[:2] for c in calls] == [("calibrate_deskew", "local-rank-0")], calls


def test_resident_shards_refuse_what_rank_0s_rows_leave_undecided(tmp_path, gpu):
    g = load_case("nrzi9_deskew_long")
    kw = _opts_of(g)
    kw.pop("subsample")
    _, rank_fn = _resident_sharded(g["hdr"], g["rows"], 2048, tmp_path, gpu, **kw)
    out = local_group.run(2, rank_fn, raise_first=False)
    assert type(out[0]) is RuntimeError and "undecided inside rank 0's 2048 rows" in str(out[0]) and "decode_file_sharded" in str(out[0])
    assert type(out[1]) is RuntimeError and "another rank failed (rank 0)" in str(out[1])
