"""k_diffz (rtfe_diffz.hip) on the MI355X: the cases of tests/test_emul_diffz_kernel.py - tests/diffz_util.py's - on the device, the spans a scan times,
and a shaped tape through streamed windows."""
import pytest

import diffz_util as dz
from readtape_amd import frontend

pytestmark = pytest.mark.gpu


def _bursts(hdr, rows, **kw):
    return frontend.FrontEnd(frontend.FrontEndConfig.from_header(hdr, find_zeros=True, **kw)).scan(rows).fetch(events=False).bursts


def test_path_reported(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    dz.check_paths_reported(frontend.FrontEnd, monkeypatch)
    hdr, rows0, rows, sites, opts = dz.shaped(2000, _bursts)
    fe = frontend.FrontEnd(frontend.FrontEndConfig.from_header(hdr, find_zeros=True, differentiate=True))
    fe.set_timing(True)
    r = fe.scan(rows).fetch()
    ms, scans = fe.kernel_ms()
    assert int(r.counts.sum()) > 100 and scans == 1
    assert ms["k_zeros"] > 0 and ms["k_decode"] == 0, ms        # (k_diffz is timed in the k_zeros span; k_decode did not run)


@pytest.mark.parametrize("mode", dz.MODES)
def test_shaped_diffz_against_the_oracle(mode, tmp_path):
    dz.check_against_oracle(mode, frontend.FrontEnd, None, tmp_path)


@pytest.mark.parametrize("ntrks", [1, 2, 7, 8, 9, 19])
def test_diffz_path_against_path(ntrks, monkeypatch):
    dz.check_track_counts(ntrks, frontend.FrontEnd, monkeypatch)


@pytest.mark.parametrize("ntrks", [9, 19])
def test_diffz_block_ends_on_the_seams(ntrks, monkeypatch):
    dz.check_block_ends(ntrks, frontend.FrontEnd, monkeypatch)


def test_diffz_flags(monkeypatch):
    dz.check_flags(frontend.FrontEnd, monkeypatch)


def test_diffz_long_flat_stretch(monkeypatch):
    dz.check_long_flat(frontend.FrontEnd, monkeypatch)


def test_diffz_exact_scans(monkeypatch):
    dz.check_exact_scans(frontend.FrontEnd, monkeypatch)


@pytest.mark.parametrize("seed,window,halo", [(2001, 1 << 12, 1 << 10), (2002, 1 << 11, 1 << 10)])
def test_diffz_in_streamed_windows(seed, window, halo, tmp_path):
    """a shaped -zeros -differentiate tape through device windows shorter than its blocks writes the .tap of the whole-tape decode"""
    from readtape_amd import ingest, pipeline, tbin
    hdr, rows0, rows, sites, opts = dz.shaped(seed, _bursts)
    kw = {"find_zeros": True, "differentiate": True}
    pipeline.decode_tape(hdr, rows, str(tmp_path / "whole.tap"), **kw)
    path = str(tmp_path / "t.tbin")
    tbin.write_tbin(path, hdr, rows)
    st = ingest.decode_file_streaming(path, str(tmp_path / "s.tap"), window_rows=window, halo_rows=halo, replay_threads=4, replay_split=3, cfgkw=kw)
    assert open(tmp_path / "s.tap", "rb").read() == open(tmp_path / "whole.tap", "rb").read()
    assert st["rows"] == rows.shape[0] and st["windows"] >= 3
