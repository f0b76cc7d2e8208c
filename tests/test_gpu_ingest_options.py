"""GPU: the streaming reader's options (readtape_amd/ingest.py) - a header without a density, -deskew, -subsample, -skip - against the golden tapes'
reference output and against the resident decode, through windows far shorter than the tape; and rtfe_decimate_rows, the kernel that thins a raw
window, at the shapes of tests/decimate_util.py."""
import dataclasses

import numpy as np
import pytest

import decimate_util as du
from golden_util import load_case
from readtape_amd import frontend, ingest, pipeline, synth, tbin

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


# ---- the kernel ----

def _gpu_call(torch, lib):
    st = torch.cuda.current_stream().cuda_stream

    def call(raw, nrows, first, step, buf, pad, kept, mark):
        ntrks = raw.shape[1]
        d_in = torch.from_numpy(raw).cuda() if raw.size else torch.zeros((8, ntrks), dtype=torch.int16, device="cuda")
        store = torch.empty(buf.nbytes + 32, dtype=torch.uint8, device="cuda")
        off = -(store.data_ptr() + pad * 2 * ntrks) % 16                     # the first row to write on a 16-byte boundary, guard rows in front of it
        view = store[off: off + buf.nbytes]
        view.copy_(torch.from_numpy(buf.view(np.uint8).reshape(-1)))
        d_mark = torch.from_numpy(mark).cuda()
        rc = lib.rtfe_decimate_rows(d_in.data_ptr(), nrows, ntrks, first, step, view.data_ptr() + pad * 2 * ntrks, kept, d_mark.data_ptr(), st)
        torch.cuda.synchronize()
        return rc, view.cpu().numpy().view(np.int16).reshape(buf.shape), d_mark.cpu().numpy()
    return call


def test_decimate_rows_at_every_shape(gpu):
    lib = frontend._load_library()
    assert du.check_all(_gpu_call(gpu, lib), lib.rtfe_decimate_span_rows) > 1000


def test_decimate_rows_past_two_gigabytes(gpu):
    """Byte offsets beyond 2^31 on both sides of a workgroup's arithmetic: 2.2 GB of nineteen-track rows, every fourth kept, a marker behind the 2^31st byte."""
    torch = gpu
    lib, be = frontend._load_library(), frontend.TorchBackend()
    ntrks, step, first = 19, 4, 3
    nrows = (1 << 31) // (2 * ntrks) + 1_000_003
    raw = torch.randint(-32767, 32768, (nrows, ntrks), dtype=torch.int16, device="cuda")
    m = nrows - 77_777
    assert m * 2 * ntrks > (1 << 31)
    raw[m, 0] = -32768
    raw[m - 5, 3] = -32768
    out = torch.full((len(range(first, nrows, step)) + 8, ntrks), 0x5A5A, dtype=torch.int16, device="cuda")
    d_mark = be.empty(16)
    n = frontend.decimate_rows(lib, be, raw, nrows, first, step, out[:-8], d_mark)
    assert n == out.shape[0] - 8 and torch.equal(out[:n], raw[first::step]) and bool((out[n:] == 0x5A5A).all())
    assert int(be.to_numpy(d_mark, np.int64)[0]) == m


# ---- the streaming reader ----

def _opts_of(g):
    """The golden's reference options as tests/test_gpu_parity.py maps them (test_emul_replay.decode_case)."""
    o = g["oracle_opts"]
    return dict(opts=pipeline.DecodeOptions(multiple_tries="-m" in o, correct="-correct" in o), deskew="-deskew" in o,
                subsample=next((int(a[11:]) for a in o if a.startswith("-subsample=")), 1))


_resident_cache = {}


def _resident(name, tmp_path):
    """(stats, .tap) of the resident decode of a golden tape - computed once."""
    if name not in _resident_cache:
        g = load_case(name)
        tap = str(tmp_path / "resident.tap")
        stats, _ = pipeline.decode_tape(g["hdr"], g["rows"], tap, **_opts_of(g))
        _resident_cache[name] = (stats, open(tap, "rb").read())
    return _resident_cache[name]


def _stream(hdr, rows, tmp_path, **kw):
    path, tap = str(tmp_path / "t.tbin"), str(tmp_path / "s.tap")
    with open(path, "wb") as f:                           # (not tbin.write_tbin: some of these payloads carry an end marker inside)
        f.write(tbin.pack_header(hdr))
        f.write(np.ascontiguousarray(rows, dtype="<i2").tobytes())
        f.write(np.array([tbin.END_MARK], dtype="<i2").tobytes())
    st = ingest.decode_file_streaming(path, tap, **kw)
    return open(tap, "rb").read(), st


@pytest.mark.parametrize("name", ["nrzi9_nobpi", "nrzi9_nobpi_short"])
def test_a_header_without_density(name, tmp_path, gpu):
    g = load_case(name)
    assert not g["hdr"].bpi > 0
    tap, st = _stream(g["hdr"], g["rows"], tmp_path, window_rows=1 << 14, halo_rows=1 << 10, **_opts_of(g))
    assert tap == g["tap"]
    assert st["bpi"] == _resident(name, tmp_path)[0]["bpi"] > 0
    assert st["rows"] == st["raw_rows"] == g["rows"].shape[0] and st["windows"] >= (3 if name == "nrzi9_nobpi" else 1)


def test_a_pe_header_without_density_is_refused_as_the_resident_decode_refuses_it(tmp_path, gpu):
    tape = synth.pe_tape(seed=5, nblocks=2)
    hdr = dataclasses.replace(tape.spec.header(), bpi=0.0)
    with pytest.raises(NotImplementedError, match="NRZI only"):
        pipeline.decode_tape(hdr, tape.rows, str(tmp_path / "r.tap"))
    with pytest.raises(NotImplementedError, match="NRZI only"):
        _stream(hdr, tape.rows, tmp_path, window_rows=1 << 14, halo_rows=1 << 10)


@pytest.mark.parametrize("name,window,prepass", [("nrzi9_deskew_long", 1 << 14, 8192), ("nrzi9_deskew_long", 1 << 14, 1 << 22), ("gcr_deskew", 1 << 13, 1 << 22),
                                                 ("nrzi9_nobpi_deskew", 1 << 14, 1 << 22), ("nrzi9_nobpi_deskew", 1 << 14, 4096)])
def test_deskew(name, window, prepass, tmp_path, gpu, monkeypatch):
    """The pre-passes on a prefix read the reader's way decide what the resident decode decides: the reference's .tap, the resident decode's delays."""
    g = load_case(name)
    want_stats, _ = _resident(name, tmp_path)
    undecided = []
    for fn_name in ("calibrate_deskew", "detect_density"):
        def counted(*a, _fn=getattr(pipeline, fn_name), _name=fn_name, **kw):
            r = _fn(*a, **kw)
            if r is None:
                undecided.append((_name, int(a[1].shape[0])))
            return r
        monkeypatch.setattr(pipeline, fn_name, counted)
    tap, st = _stream(g["hdr"], g["rows"], tmp_path, window_rows=window, halo_rows=1 << 10, prepass_rows=prepass, **_opts_of(g))
    assert tap == g["tap"]
    assert st["skew"] == want_stats["skew"] and st["skew"] is not None and st["bpi"] == want_stats["bpi"]
    assert st["windows"] >= 3
    if prepass < (1 << 14):
        assert undecided and all(n < g["rows"].shape[0] for _, n in undecided), undecided      # the prefix had to grow at least once
    else:
        assert not undecided


def test_given_delays_run_no_prepass(tmp_path, gpu, monkeypatch):
    g = load_case("nrzi9_deskew_long")
    want_stats, _ = _resident("nrzi9_deskew_long", tmp_path)

    def never(*a, **kw):
        raise AssertionError("a pre-pass ran")
    monkeypatch.setattr(pipeline, "calibrate_deskew", never)
    monkeypatch.setattr(pipeline, "detect_density", never)
    tap, st = _stream(g["hdr"], g["rows"], tmp_path, window_rows=1 << 14, halo_rows=1 << 10, deskew=True, skew=want_stats["skew"])
    assert tap == g["tap"] and st["skew"] == want_stats["skew"]


def test_subsample_golden(tmp_path, gpu):
    g = load_case("nrzi9_sub2")
    kw = _opts_of(g)
    assert kw["subsample"] == 2
    tap, st = _stream(g["hdr"], g["rows"], tmp_path, window_rows=4096, halo_rows=1 << 10, **kw)
    assert tap == g["tap"]
    assert st["rows"] == g["rows"].shape[0] // 2 and st["raw_rows"] == st["rows"] * 2 and st["windows"] >= 3


@pytest.fixture(scope="module")
def oversampled():
    """A dozen NRZI blocks sampled every 320 ns: four times the usual rate (the reference's banner: "excessive samples per bit; consider using the
    -subsample option").  Blocks up to 900 bytes: longer than the halos below, so halos have to grow."""
    spec = synth.TapeSpec(mode=tbin.MODE_NRZI, ntrks=9, bpi=800.0, ips=50.0, tdelta_ns=320, maxvolts=4.4, pulse_w=0.22, seed=83)
    rng = np.random.default_rng(83)
    items = [("block", p) for p in synth.random_payloads(rng, 12, 200, 900)]
    items.insert(5, ("mark",))
    return synth.make_tape(spec, items, gap_samples=12000)


_want_cache = {}


def _want(hdr, rows, n, tmp_path, key):
    """The resident decode of `rows` with subsample n (which tests/golden/case_nrzi9_sub2 pins to the reference) - computed once per key."""
    if key not in _want_cache:
        tap = str(tmp_path / "want.tap")
        stats, _ = pipeline.decode_tape(hdr, rows, tap, subsample=n)
        _want_cache[key] = (open(tap, "rb").read(), stats)
    return _want_cache[key]


@pytest.mark.parametrize("n", [2, 3])
def test_subsample_equals_the_resident_decode(n, oversampled, tmp_path, gpu):
    hdr = dataclasses.replace(oversampled.spec.header(), tdelta_ns=320 * n)      # (the header's tdelta is the time between USED rows)
    want, stats = _want(hdr, oversampled.rows, n, tmp_path, ("whole", n))
    assert stats["blocks"] == 12 and stats["tapemarks"] == 1
    tap, st = _stream(hdr, oversampled.rows, tmp_path, subsample=n, window_rows=1 << 15, halo_rows=1 << 12, replay_threads=1 if n == 2 else 4,
                      replay_split=1 if n == 2 else 2)
    assert tap == want
    assert st["rows"] == oversampled.rows.shape[0] // n and st["windows"] >= 3 and st["blocks"] == 12
    assert st["retries"] > 0                               # a halo had to grow: the longer window was thinned too


@pytest.mark.parametrize("where", ["skipped", "kept", "halo_skipped", "halo_kept"])
def test_subsample_with_an_end_marker_inside_the_payload(where, oversampled, tmp_path, gpu):
    """The data end at the first RAW row whose head-0 sample is the marker, whichever place in its group it has (src/readtape.c:1407-1413)."""
    n, win, halo = 2, 1 << 15, 1 << 12
    hdr = dataclasses.replace(oversampled.spec.header(), tdelta_ns=320 * n)
    used = {"skipped": 3 * win + win * 5 // 8, "kept": 3 * win + win * 5 // 8, "halo_skipped": 2 * win + 700, "halo_kept": 4 * win + 4090}[where]
    m = used * n + (n - 1 if where.endswith("kept") else 0)                  # (of every n raw rows the last is the used one)
    assert m + 2 * n * win < oversampled.rows.shape[0]                      # (windows behind the marker exist: they must decode nothing)
    rows = oversampled.rows.copy()
    rows[m, 0] = tbin.END_MARK
    want, _ = _want(hdr, oversampled.rows[:m], n, tmp_path, ("cut", m))
    tap, st = _stream(hdr, rows, tmp_path, subsample=n, window_rows=win, halo_rows=halo)
    assert st["rows"] == m // n == used and st["raw_rows"] == used * n
    assert tap == want and len(want) > 1000


def test_skip(tmp_path, gpu):
    """-skip: the decode of rows[skip:] - a skip that is a multiple of neither 1024 nor the subsampling step, and a marker among the skipped rows is not looked at."""
    tape = synth.nrzi_tape(seed=84, nblocks=20, minlen=200, maxlen=900, marks_every=6, gap_samples=3000)
    hdr = tape.spec.header()
    skip = 1531
    want_tap = str(tmp_path / "w.tap")
    pipeline.decode_tape(hdr, tape.rows[skip:], want_tap)
    rows = tape.rows.copy()
    rows[777, 0] = tbin.END_MARK
    tap, st = _stream(hdr, rows, tmp_path, skip=skip, window_rows=1 << 15, halo_rows=1 << 12)
    assert tap == open(want_tap, "rb").read() and len(tap) > 1000
    assert st["rows"] == tape.rows.shape[0] - skip and st["raw_rows"] == tape.rows.shape[0] and st["windows"] >= 3


def test_skip_with_subsample(oversampled, tmp_path, gpu):
    n, skip = 2, 1531
    hdr = dataclasses.replace(oversampled.spec.header(), tdelta_ns=320 * n)
    want, _ = _want(hdr, oversampled.rows[skip:], n, tmp_path, ("skip", skip))
    tap, st = _stream(hdr, oversampled.rows, tmp_path, subsample=n, skip=skip, window_rows=1 << 15, halo_rows=1 << 12)
    assert tap == want and len(want) > 1000
    assert st["rows"] == (oversampled.rows.shape[0] - skip) // n and st["raw_rows"] == skip + st["rows"] * n
