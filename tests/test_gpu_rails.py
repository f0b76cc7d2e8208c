"""The int16 rails through the amplitude detectors on the MI355X: the recorded cases, path knobs, shaped tapes and full-scale ladder of
tests/test_emul_rails.py on the device, every event field and the .tap bytes against the oracle, path against path byte for byte."""
import pytest

import rail_shapes as rs
from golden_util import load_case
from readtape_amd import frontend
from test_emul_rails import (DENSE_KNOBS, DIFF_RAIL_CASES, DENSE_RAIL_CASES, LADDER_CASES, NRZI_KNOBS, NRZI_RAIL_CASES, PEAK_RAIL_CASES, WW_RAIL_CASES, check_rails, decode_rail_case, ids,
                             ladder_case, same_results, set_knobs, shaped_case)

pytestmark = pytest.mark.gpu


def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return frontend.FrontEnd


@pytest.mark.parametrize("name", PEAK_RAIL_CASES)
def test_rail_cases_against_the_oracle(name, tmp_path):
    g = load_case(name)
    stats, st, res = check_rails(_gpu(), g["hdr"], g["rows"], g["oracle_opts"], str(tmp_path))
    if "sparse" in name:
        rail = rs.rail_bursts(g["rows"], res.bursts[:res.nbursts])
        assert 0 < rail.sum() and st["redone"] == rail.sum()


@pytest.mark.parametrize("knobs", NRZI_KNOBS, ids=ids)
@pytest.mark.parametrize("name", NRZI_RAIL_CASES)
def test_nrzi_rail_cases_on_every_path(name, knobs, tmp_path, monkeypatch):
    set_knobs(monkeypatch, knobs)
    g = load_case(name)
    check_rails(_gpu(), g["hdr"], g["rows"], g["oracle_opts"], str(tmp_path))


@pytest.mark.parametrize("knobs", DENSE_KNOBS, ids=ids)
@pytest.mark.parametrize("name", DENSE_RAIL_CASES)
def test_gcr_pe_rail_cases_on_every_path(name, knobs, tmp_path, monkeypatch):
    set_knobs(monkeypatch, knobs)
    g = load_case(name)
    check_rails(_gpu(), g["hdr"], g["rows"], g["oracle_opts"], str(tmp_path))


@pytest.mark.parametrize("name", PEAK_RAIL_CASES)
def test_rail_cases_path_against_path(name, monkeypatch):
    g = load_case(name)
    same_results(_gpu(), g["hdr"], g["rows"], g["oracle_opts"], monkeypatch, [{}] + (NRZI_KNOBS if name.startswith("nrzi") else DENSE_KNOBS))


@pytest.mark.parametrize("name", PEAK_RAIL_CASES + DIFF_RAIL_CASES)
def test_rail_cases_tap_bytes_match_the_reference(name, tmp_path):
    _gpu()
    g = load_case(name)
    tap, diffs = decode_rail_case(g, tmp_path, None)
    assert tap == g["tap"] and not diffs, diffs


@pytest.mark.parametrize("chunk_rows", [4096, 300])
@pytest.mark.parametrize("name", WW_RAIL_CASES)
def test_whirlwind_rail_cases_tap_bytes_match_the_reference(name, chunk_rows, tmp_path):
    _gpu()
    g = load_case(name)
    tap, diffs = decode_rail_case(g, tmp_path, None, chunk_rows)
    assert tap == g["tap"] and not diffs, diffs


@pytest.mark.parametrize("name,mv,invert", LADDER_CASES)
def test_full_scale_ladder(name, mv, invert, tmp_path):
    ladder_case(_gpu(), name, mv, invert, str(tmp_path))


@pytest.mark.parametrize("seed", range(1, 25))
def test_shaped_rails_against_the_oracle(seed, tmp_path):
    shaped_case(_gpu(), seed, str(tmp_path))


@pytest.mark.parametrize("kind", rs.KINDS)
@pytest.mark.parametrize("how", ["sparse", "x2", "x4"])
def test_shaped_rails_of_every_kind_inverted(kind, how, tmp_path):
    over = dict(kind=kind, how=how, invert=True, skew=kind == "nrzi9", m=False, fluxdir="auto" if kind == "ww" else None)
    shaped_case(_gpu(), 11, str(tmp_path), over)
