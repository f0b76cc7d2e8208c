"""The quiet map (k_quiet, k_sift / k_sift_s + k_qpack, k_dseg) and the burst table (k_bursts, k_bursts_cnt / _emit / _tail) through the CPU emulator against
the plain reference of tests/burst_ref.py: every compared field of every burst, no tolerance.  The shapes are tests/burst_shapes.py's; each runs with the
single-workgroup search and with a workgroup per round of 1, 3 and 64 words (a fresh handle per setting), with first_is_tape_start on and off and with
own_rows below nrows where the shape's name says so.  tests/test_gpu_burst_table.py runs the same cases on the device."""
import pytest

import burst_shapes as bs
from emul_util import emul_frontend

_wpr_id = lambda w: "wpr_default" if w is None else f"wpr{w}"


@pytest.mark.parametrize("wpr", bs.WPRS, ids=_wpr_id)
@pytest.mark.parametrize("shape", bs.TABLE_SHAPES, ids=lambda s: s.name)
def test_emulated_burst_table(shape, wpr, monkeypatch):
    bs.check_table(shape, emul_frontend, monkeypatch, wpr)


@pytest.mark.parametrize("wpr", bs.WPRS, ids=_wpr_id)
def test_emulated_burst_table_many_bursts(wpr, monkeypatch):
    bs.check_many_bursts(emul_frontend, monkeypatch, wpr)


@pytest.mark.parametrize("shape", bs.PRODUCER_END_SHAPES, ids=lambda s: s.name)
def test_emulated_tape_end_per_producer(shape, monkeypatch):
    bs.check_table(shape, emul_frontend, monkeypatch, None)


@pytest.mark.parametrize("producer,ntrks", bs.THRESHOLD_CASES)
def test_emulated_quiet_threshold(producer, ntrks, monkeypatch):
    bs.check_threshold(producer, ntrks, emul_frontend, monkeypatch)
