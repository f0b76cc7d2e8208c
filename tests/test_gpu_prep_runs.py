"""k_prep by runs of consecutive tiles of one stream (RTFE_PREP_RUN) on the MI355X: every event against the oracle for runs of 1, 2, 3 tiles, the default and the
longest, on the tapes of tests/test_emul_prep_runs.py (which asserts, on the emulator, that they reach the seams of a run)."""
import numpy as np
import pytest

from fuzz_util import base_tape
from parity_util import check_tape, config_for, oracle_attempts
from readtape_amd import frontend, synth

pytestmark = pytest.mark.gpu

RUNS = [1, 2, 3, None, 32]


def _check(hdr, rows, opts, run, knobs, tmp_path, monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    if run is None:
        monkeypatch.delenv("RTFE_PREP_RUN", raising=False)
    else:
        monkeypatch.setenv("RTFE_PREP_RUN", str(run))
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    att = oracle_attempts(hdr, rows, opts, str(tmp_path))
    fe = frontend.FrontEnd(config_for(hdr, opts))
    for rep in range(2):
        msgs, stats = check_tape(fe, hdr, rows, att)
        assert not msgs, "\n".join(msgs[:12])
        assert stats["events"] > 0


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("knobs", [{}, {"RTFE_PK_SLOT": "64"}, {"RTFE_CCAP": "200"}])
def test_clean_tape(run, knobs, tmp_path, monkeypatch):
    tape, opts = base_tape("nrzi9", 3, 5.0)
    rows = np.ascontiguousarray(tape.rows[:25 * 896 - 100]) if not knobs else tape.rows
    _check(tape.spec.header(), rows, opts, run, knobs, tmp_path, monkeypatch)


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("knobs", [{}, {"RTFE_PK_SLOT": "512"}])
def test_noisy_tape(run, knobs, tmp_path, monkeypatch):
    tape = synth.nrzi_tape(seed=12, nblocks=10, minlen=150, maxlen=400, gap_samples=3000, noise_mv=60.0, ntrks=9)
    _check(tape.spec.header(), tape.rows, [], run, knobs, tmp_path, monkeypatch)


@pytest.mark.parametrize("run", RUNS)
def test_pe_on_the_peak_path(run, tmp_path, monkeypatch):
    tape, opts = base_tape("pe", 4, 10.0)
    _check(tape.spec.header(), tape.rows, opts, run, {"RTFE_PEAK_PATH": "1"}, tmp_path, monkeypatch)
