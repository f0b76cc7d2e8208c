"""The shaped -zeros / -zeros -differentiate tapes of tests/zeros_shapes.py on the MI355X, end to end against the oracle, path against path over track
counts 2 .. 19, through streamed windows, and the threshold ladder and rails of tests/test_emul_zeros_shapes.py on the device."""
import dataclasses

import numpy as np
import pytest

import zeros_shapes as zs
import zeros_util
from readtape_amd import frontend
from test_emul_zeros_shapes import MIN_SEAMS, _ladder, _rail_tape, inverted_rail_case

pytestmark = pytest.mark.gpu


def _bursts(hdr, rows, **kw):
    fe = frontend.FrontEnd(frontend.FrontEndConfig.from_header(hdr, find_zeros=True, **kw))
    return fe.scan(rows).fetch(events=False).bursts


@pytest.mark.parametrize("mode", ["zeros", "diffz", "invert"])
def test_shaped_zeros_against_the_oracle(mode, tmp_path):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    cov, changed = {}, 0
    seeds = range(1000, 1014)
    for seed in seeds:
        hdr, rows0, rows, sites, opts = zs.shaped(seed, _bursts, diff=mode == "diffz")
        opts = opts + (["-invert"] if mode == "invert" else [])
        msgs, b = zs.e2e(hdr, rows, opts, str(tmp_path / f"s{seed}"))
        assert not msgs, f"seed {seed} {zs.draw(seed)} {opts}: " + "\n".join(str(m) for m in msgs[:8])
        _, b0 = zs.e2e(hdr, rows0, opts, str(tmp_path / f"u{seed}"))
        changed += b.size != b0.size or not np.array_equal(b["timenow_ns"], b0["timenow_ns"])
        for k, v in zs.coverage(sites, hdr, rows.shape[0], _bursts(hdr, rows)).items():
            cov[k] = cov.get(k, 0) + v
    shapes = zs.DIFF_SHAPES + ("Z-zero", "Z-flicker", "Z-rail") if mode == "diffz" else zs.SHAPES
    for c in shapes + zs.SEAMS:
        assert cov.get(c, 0) >= 3 * MIN_SEAMS, (c, cov)
    assert changed >= len(seeds) // 2


@pytest.mark.parametrize("ntrks", [2, 7, 8, 9, 19])
@pytest.mark.parametrize("seed", [11, 12])
def test_shaped_zeros_path_against_path(ntrks, seed, monkeypatch):
    hdr, rows0, rows, sites, opts = zs.shaped(seed, _bursts, ntrks=ntrks)
    variants = [{}, {"RTFE_ZEROS_KERNEL": "0"}, {"RTFE_ZC_PARALLEL": "0"}, {"RTFE_ZC_WARM": "16"}, {"RTFE_ZC_WARM": "64"}]
    out = zeros_util.scan_variants(frontend.FrontEnd, hdr, rows, monkeypatch, variants)
    assert out[0].nbursts >= 2
    for r in out[1:]:
        zeros_util.same_scan(out[0], r, ntrks)
    cov = zs.coverage(sites, hdr, rows.shape[0], out[0].bursts)
    for c in ("zp_sub", "zp_warm", "zc_sub") + (("odd_col", "unaligned_pair") if ntrks & 1 else ()):
        assert cov.get(c, 0) >= 2, (c, cov)


@pytest.mark.parametrize("seed,window,halo", [(1001, 1 << 12, 1 << 10), (1002, 1 << 11, 1 << 10)])
def test_shaped_zeros_in_streamed_windows(seed, window, halo, tmp_path):
    """a shaped -zeros tape through device windows shorter than its blocks writes the .tap of the whole-tape decode"""
    from readtape_amd import ingest, pipeline, tbin
    hdr, rows0, rows, sites, opts = zs.shaped(seed, _bursts)
    pipeline.decode_tape(hdr, rows, str(tmp_path / "whole.tap"), find_zeros=True)
    want = open(tmp_path / "whole.tap", "rb").read()
    path = str(tmp_path / "t.tbin")
    tbin.write_tbin(path, hdr, rows)
    st = ingest.decode_file_streaming(path, str(tmp_path / "s.tap"), window_rows=window, halo_rows=halo, replay_threads=4, replay_split=3, cfgkw={"find_zeros": True})
    assert open(tmp_path / "s.tap", "rb").read() == want
    assert st["rows"] == rows.shape[0] and st["windows"] >= 3


@pytest.mark.parametrize("invert", [False, True], ids=["k_zeros", "k_decode"])
def test_maxvolts_where_no_code_reaches_the_threshold(invert, tmp_path):
    hdr, rows = _rail_tape()
    for mv in (0.2, 0.2000001):
        msgs, b = zs.e2e(dataclasses.replace(hdr, maxvolts=mv), rows, ["-zeros"] + (["-invert"] if invert else []), str(tmp_path / str(mv)))
        assert not msgs, "\n".join(str(m) for m in msgs[:8])
        assert (b.size < 10) if mv == 0.2 else (b.size > 4000)


@pytest.mark.parametrize("mv", [0.15, 0.199, 0.2, 0.2000001, 0.37, 7000.0])
@pytest.mark.parametrize("invert", [False, True], ids=["k_zeros", "k_decode"])
def test_threshold_ladder(mv, invert, tmp_path):
    hdr, rows = _rail_tape(scale=4 if mv < 1 else 1)
    h = dataclasses.replace(hdr, maxvolts=mv)
    P = zs.zc_peak_code(mv)
    rows = _ladder(h, rows, min(P, 32767) if P > 2 else 3, np.random.default_rng(int(mv * 1000)))
    msgs, b = zs.e2e(h, rows, ["-zeros"] + (["-invert"] if invert else []), str(tmp_path))
    assert not msgs, "\n".join(str(m) for m in msgs[:8])


@pytest.mark.parametrize("opts", [["-zeros", "-invert"], ["-zeros", "-invert", "-differentiate"]])
def test_inverted_negative_rail(opts, tmp_path):
    inverted_rail_case(opts, tmp_path, None)
