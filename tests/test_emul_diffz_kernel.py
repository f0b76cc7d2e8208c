"""k_diffz (rtfe_diffz.hip: -zeros -differentiate as a three-state transducer, a lane per sub-segment and track) through the CPU emulator: the path a
handle reports, shaped tapes end to end against the oracle, k_diffz against k_decode's literal walk byte for byte at its seams, and through fragments.
The cases are tests/diffz_util.py's; tests/test_gpu_diffz_kernel.py runs the same ones on the device."""
import pytest

import diffz_util as dz
from diffz_util import emul_frontend


def _bursts(hdr, rows, **kw):
    from readtape_amd import frontend
    return emul_frontend(frontend.FrontEndConfig.from_header(hdr, find_zeros=True, **kw)).scan(rows).fetch(events=False).bursts


def test_seam_constants_match_the_kernel():
    """the placement aims at the seams the kernel has: a retune of kDzHead / kDzSub / kDzThreads fails here"""
    head, sub, threads, chunk = dz.kernel_constants()
    assert (head, sub, threads) == (dz.KDZ_HEAD, dz.KDZ_SUB, dz.KDZ_THREADS)
    assert chunk == "kDzThreads / ntrks"
    assert [dz.chunk_subs(n) for n in (1, 2, 7, 9, 19)] == [256, 128, 36, 28, 13]
    assert dz.seams_of(60, 66, 9, [(0, 5000)]) == {"dz_head"} and dz.seams_of(64 + 28 * 128 - 1, 64 + 28 * 128, 9, [(0, 5000)]) == {"dz_chunk"}
    assert dz.seams_of(64 + 38 * 128 - 3, 64 + 38 * 128 + 2, 9, [(0, 5000)]) == {"dz_sub", "dz_last"}
    assert dz.seams_of(64 + 38 * 128 - 3, 64 + 38 * 128 + 2, 9, [(0, 64 + 39 * 128)]) == {"dz_sub"}


def test_path_reported(monkeypatch):
    dz.check_paths_reported(emul_frontend, monkeypatch)


@pytest.mark.parametrize("mode", dz.MODES)
def test_shaped_diffz_against_the_oracle(mode, tmp_path):
    dz.check_against_oracle(mode, emul_frontend, emul_frontend, tmp_path)


@pytest.mark.parametrize("ntrks", [1, 2, 7, 8, 9, 19])
def test_diffz_path_against_path(ntrks, monkeypatch):
    dz.check_track_counts(ntrks, emul_frontend, monkeypatch)


@pytest.mark.parametrize("ntrks", [9, 19])
def test_diffz_block_ends_on_the_seams(ntrks, monkeypatch):
    dz.check_block_ends(ntrks, emul_frontend, monkeypatch)


def test_diffz_flags(monkeypatch):
    dz.check_flags(emul_frontend, monkeypatch)


def test_diffz_long_flat_stretch(monkeypatch):
    dz.check_long_flat(emul_frontend, monkeypatch)


def test_diffz_exact_scans(monkeypatch):
    dz.check_exact_scans(emul_frontend, monkeypatch)


@pytest.mark.parametrize("seed,window,halo", [(2001, 1 << 12, 1 << 10), (2002, 1 << 11, 1 << 10)])
def test_diffz_in_fragments(seed, window, halo, tmp_path):
    """a shaped tape decoded as fragments shorter than its blocks writes the .tap of the whole-tape decode (the device test streams the same windows)"""
    from readtape_amd import pipeline
    hdr, rows0, rows, sites, opts = dz.shaped(seed, _bursts)
    kw = {"find_zeros": True, "differentiate": True}
    pipeline.decode_tape(hdr, rows, str(tmp_path / "whole.tap"), fe_factory=emul_frontend, **kw)
    n = rows.shape[0]
    spans = [(lo, min(lo + window, n)) for lo in range(0, n, window)]
    st = pipeline.decode_tape_fragments(hdr, rows, str(tmp_path / "f.tap"), spans, fe_factory=emul_frontend, halo_rows=halo, cfgkw=kw)
    assert open(tmp_path / "f.tap", "rb").read() == open(tmp_path / "whole.tap", "rb").read()
    assert len(st) >= 3
