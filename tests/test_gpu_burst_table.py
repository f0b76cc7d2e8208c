"""The quiet map and the burst table on the MI355X against the plain reference of tests/burst_ref.py: the cases of tests/test_emul_burst_table.py -
tests/burst_shapes.py's - on the device, and one shape the emulator cannot afford (2^24 + 8192 rows: the single workgroup's second round)."""
import pytest

import burst_shapes as bs
from readtape_amd import frontend

pytestmark = pytest.mark.gpu

_wpr_id = lambda w: "wpr_default" if w is None else f"wpr{w}"


@pytest.mark.parametrize("wpr", bs.WPRS, ids=_wpr_id)
@pytest.mark.parametrize("shape", bs.TABLE_SHAPES, ids=lambda s: s.name)
def test_burst_table(shape, wpr, monkeypatch):
    bs.check_table(shape, frontend.FrontEnd, monkeypatch, wpr)


@pytest.mark.parametrize("wpr", bs.WPRS, ids=_wpr_id)
def test_burst_table_many_bursts(wpr, monkeypatch):
    bs.check_many_bursts(frontend.FrontEnd, monkeypatch, wpr)


@pytest.mark.parametrize("shape", bs.PRODUCER_END_SHAPES, ids=lambda s: s.name)
def test_tape_end_per_producer(shape, monkeypatch):
    bs.check_table(shape, frontend.FrontEnd, monkeypatch, None)


@pytest.mark.parametrize("producer,ntrks", bs.THRESHOLD_CASES)
def test_quiet_threshold(producer, ntrks, monkeypatch):
    bs.check_threshold(producer, ntrks, frontend.FrontEnd, monkeypatch)


def test_burst_table_second_round_of_the_single_workgroup(monkeypatch):
    bs.check_big(frontend.FrontEnd, monkeypatch)
