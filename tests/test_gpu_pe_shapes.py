"""Where a PE track's preamble ends, on the MI355X: the tapes of tests/test_emul_pe_shapes.py (tests/pe_shapes.py, the seeds whose counters the emulator test
asserts from the oracle alone - asserted again here before parity) through the C ABI, every event field against the oracle, with and without -m, two scans a
handle, on the dense path, on k_decode, on the peak path (k_gain's mirror) with and without its lean step, and with RTFE_DS_LEAN=0; path against path byte for
byte; a fragment cut and a streamed window's edge inside a preamble; and the recorded cases end to end against the unmodified reference's .tap.  The device's
own lines - fast_rcp, the packed and LDS-typed lines, readfirstlane - are code the emulator does not run: these tests are what sees them."""
import numpy as np
import pytest

import pe_shapes as ps
import pe_util as pu
from readtape_amd import frontend

pytestmark = pytest.mark.gpu


def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return frontend.FrontEnd


@pytest.mark.parametrize("knobs", pu.PATH_KNOBS, ids=pu.ids)
@pytest.mark.parametrize("m", [False, True], ids=["one_set", "m"])
@pytest.mark.parametrize("cls", ps.CLASSES)
def test_every_event_field_against_the_oracle(cls, m, knobs, monkeypatch):
    make = _gpu()
    pu.assert_class(cls, pu.class_totals(cls, m), m)
    pu.set_knobs(monkeypatch, knobs)
    assert pu.check_class(make, cls, m) > 5000


@pytest.mark.parametrize("knobs", [{}, {"RTFE_DENSE_PATH": "0"}, {"RTFE_PEAK_PATH": "1"}], ids=pu.ids)
@pytest.mark.parametrize("opt", ["invert", "skew", "invert_skew_m"])
@pytest.mark.parametrize("cls", ps.CLASSES)
def test_the_options_of_every_class(cls, opt, knobs, monkeypatch):
    make = _gpu()
    kw = dict(invert="invert" in opt, skew="skew" in opt, m=opt.endswith("_m"))
    tot = pu.class_totals(cls, **kw)
    assert tot["events"] > 5000 and tot["tracks"] >= 36
    pu.set_knobs(monkeypatch, knobs)
    assert pu.check_class(make, cls, **kw) > 5000


@pytest.mark.parametrize("cls", ps.CLASSES)
def test_path_against_path_on_the_same_rows(cls, monkeypatch):
    make = _gpu()
    label, tp, att, win = pu.tapes_of(cls, 1, m=True)[0]
    pu.same_results(make, ps.config(tp), tp["rows"], monkeypatch, pu.PATH_KNOBS + [{"RTFE_DENSE_DEDUP": "0"}])


@pytest.mark.parametrize("peak", [40, 66, 70, 71])
def test_a_fragment_cut_inside_a_preamble(peak):
    make = _gpu()
    (_, tp, att, _), = pu.tapes_of("P-length", 1)
    assert pu.fragments_case(make, tp, peak) > 5000


@pytest.mark.parametrize("m", [False, True], ids=["one_set", "m"])
def test_a_streamed_windows_edge_inside_a_preamble(m, tmp_path):
    """the streaming reader's first window ends on peak 66 of a 37-bit preamble (every later edge a multiple of it), halos shorter than the block: the .tap of
    the whole-tape decode, whose events the tests above hold against the oracle"""
    from readtape_amd import ingest, pipeline, tbin
    _gpu()
    (_, tp, att, _), = pu.tapes_of("P-length", 1, m)
    rows, cut = pu.preamble_cut(tp, 66)
    opts = pipeline.DecodeOptions(multiple_tries=m)
    pipeline.decode_tape(tp["hdr"], rows, str(tmp_path / "whole.tap"), opts=opts)
    want = open(tmp_path / "whole.tap", "rb").read()
    path = str(tmp_path / "t.tbin")
    tbin.write_tbin(path, tp["hdr"], rows)
    st = ingest.decode_file_streaming(path, str(tmp_path / "s.tap"), window_rows=cut, halo_rows=1 << 10, replay_threads=4, replay_split=3, opts=opts)
    assert len(want) > 150, "the tape decodes to next to nothing: the comparison would be vacuous"
    assert open(tmp_path / "s.tap", "rb").read() == want
    assert st["rows"] == rows.shape[0] and st["windows"] >= 3


@pytest.mark.parametrize("knobs", [{}, {"RTFE_DENSE_PATH": "0"}, {"RTFE_PEAK_PATH": "1"}], ids=pu.ids)
@pytest.mark.parametrize("name", ["pe_pre35", "pe_pre36", "pe_pre20", "pe_mark", "pe_clk"])
def test_tap_bytes_of_the_recorded_cases(name, knobs, tmp_path, monkeypatch):
    """P-length, P-mark and P-clk end to end: front end -> event replay -> block decoders -> the unmodified reference's .tap, transitions and block lines"""
    from golden_util import load_case
    from test_emul_replay import decode_case
    _gpu()
    pu.set_knobs(monkeypatch, knobs)
    g = load_case(name)
    tap, stats = decode_case(g, tmp_path, None)
    assert tap == g["tap"]
    assert stats["agc_mismatches"] == 0 and stats["events_delivered"] > 0 and not stats["event_diffs"], stats
