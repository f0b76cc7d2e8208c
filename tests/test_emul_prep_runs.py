"""k_prep by runs of consecutive tiles of one stream (RTFE_PREP_RUN), on the CPU emulator: the events against the oracle, and what kCrClear promises re-derived from
the finished streams (RTFE_PREP_CHECK), for runs of 1, 2, 3 tiles, the default and the longest - on tapes that reach, and are asserted to reach, the seams of a run: a last run
that is shorter than the others, empty lists inside a run and as its last, lists of more than 32 records, lists that outgrew their slot inside a run and directly
behind one, deferred candidates as a record's successor inside a list, across a list's end and across a run's end, a stream that outgrew its capacity.
(RTFE_PREP_CHECK=2 makes the emulator count these from the directory and the pool: the "prep_shapes:" line.)"""
import re

import numpy as np
import pytest

from emul_util import emul_frontend
from readtape_amd import synth
from fuzz_util import base_tape
from parity_util import check_tape, config_for, oracle_attempts

DEFAULT_RUN = 8
RUNS = [1, 2, 3, None, 32]      # None: RTFE_PREP_RUN unset; 32: the longest


def _tape(kind, seed, noise_mv, rows_cut=None):
    tape, opts = base_tape(kind, seed, noise_mv)
    rows = tape.rows if rows_cut is None else np.ascontiguousarray(tape.rows[:rows_cut])
    return tape.spec.header(), rows, opts


def _run(hdr, rows, opts, run, knobs, tmp_path, monkeypatch, capfd, allow_redo=False):
    """one scan pair under the knobs; returns the counts of the prep_shapes line"""
    monkeypatch.setenv("RTFE_PREP_CHECK", "2")
    if run is None:
        monkeypatch.delenv("RTFE_PREP_RUN", raising=False)
    else:
        monkeypatch.setenv("RTFE_PREP_RUN", str(run))
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    att = oracle_attempts(hdr, rows, opts, str(tmp_path))
    fe = emul_frontend(config_for(hdr, opts))
    capfd.readouterr()
    for rep in range(2):                                  # (the second scan runs under the floor the first one learned)
        msgs, stats = check_tape(fe, hdr, rows, att)
        assert not msgs, "\n".join(msgs[:12])
        assert stats["events"] > 0
    err = capfd.readouterr().err
    assert "prep_check: stream" not in err, err[:2000]
    lines = [ln for ln in err.splitlines() if ln.startswith("prep_shapes:")]
    assert lines
    shapes = [{k: int(v) for k, v in re.findall(r"(\w+) (\d+)", ln[len("prep_shapes:"):])} for ln in lines]
    for s in shapes:
        assert s["run"] == (DEFAULT_RUN if run is None else run)
    # (every scan's counts; a seam counts as reached if one scan of the pair reached it)
    return {k: max(s[k] for s in shapes) for k in shapes[0]}


@pytest.mark.parametrize("run", RUNS)
def test_clean_tape_short_last_run_and_empty_lists(run, tmp_path, monkeypatch, capfd):
    """the gaps between the blocks: empty lists inside a run and as a run's last; 25 tiles: not a multiple of 2, 3 or 8"""
    hdr, rows, opts = _tape("nrzi9", 3, 5.0, rows_cut=25 * 896 - 100)
    s = _run(hdr, rows, opts, run, {}, tmp_path, monkeypatch, capfd)
    r = s["run"]
    assert s["tiles"] == 25
    if r > 1:
        assert s["tiles"] % r != 0 and s["empty_in"] > 0
    if r <= DEFAULT_RUN:                                  # (the longest run, an extra: 25 tiles are less than one of it - the events alone)
        assert s["empty_last"] > 0
    assert s["over_ccap"] == 0


@pytest.mark.parametrize("run", RUNS)
def test_noisy_tape_deferred_candidates_at_every_seam(run, tmp_path, monkeypatch, capfd):
    """deferred candidates (60 mV of noise) as the successor of a plain record: inside a list, across a list's end, across a run's end"""
    tape = synth.nrzi_tape(seed=12, nblocks=10, minlen=150, maxlen=400, gap_samples=3000, noise_mv=60.0, ntrks=9)      # (ten blocks: a run's first entry is one in eight)
    s = _run(tape.spec.header(), tape.rows, [], run, {}, tmp_path, monkeypatch, capfd)
    assert s["deferred_in"] > 0 and s["long"] > 0
    if s["run"] <= DEFAULT_RUN:                           # (the longest run, an extra: four runs a stream - the events alone)
        assert s["deferred_run"] > 0
    if s["run"] > 1:
        assert s["deferred_list"] > 0


@pytest.mark.parametrize("run", RUNS)
def test_lists_of_more_than_32_records(run, tmp_path, monkeypatch, capfd):
    """PE on the peak path: a flux change every few rows - a list takes more than one round of a wave, a run more than one batch of rounds"""
    hdr, rows, opts = _tape("pe", 4, 10.0)
    s = _run(hdr, rows, opts, run, {"RTFE_PEAK_PATH": "1"}, tmp_path, monkeypatch, capfd)
    assert s["long"] > 100


@pytest.mark.parametrize("run", RUNS)
def test_lists_that_outgrew_their_slot(run, tmp_path, monkeypatch, capfd):
    """RTFE_PK_SLOT=64: four records a slot - nearly every list of a block is a marker: inside a run and directly behind one"""
    hdr, rows, opts = _tape("nrzi9", 3, 5.0)
    s = _run(hdr, rows, opts, run, {"RTFE_PK_SLOT": "64"}, tmp_path, monkeypatch, capfd)
    assert s["markers_behind"] > 0
    if s["run"] > 1:
        assert s["markers_in"] > 0


@pytest.mark.parametrize("run", RUNS)
def test_markers_behind_records(run, tmp_path, monkeypatch, capfd):
    """a noisy tape's lists of 20 to 40 records in slots of 32: lists that fit and lists that did not side by side - the last record of a list looks at a marker,
    inside a run and across a run's end"""
    tape = synth.nrzi_tape(seed=12, nblocks=10, minlen=150, maxlen=400, gap_samples=3000, noise_mv=60.0, ntrks=9)
    s = _run(tape.spec.header(), tape.rows, [], run, {"RTFE_PK_SLOT": "512"}, tmp_path, monkeypatch, capfd)
    assert s["marker_behind"] > 0
    if s["run"] > 1:
        assert s["marker_in"] > 0


@pytest.mark.parametrize("run", RUNS)
def test_stream_over_its_capacity(run, tmp_path, monkeypatch, capfd):
    """RTFE_CCAP: streams that outgrew their capacity are not built - their chains give up, the bursts are redone on the samples: the same events"""
    hdr, rows, opts = _tape("nrzi9", 3, 5.0)
    s = _run(hdr, rows, opts, run, {"RTFE_CCAP": "200"}, tmp_path, monkeypatch, capfd)
    assert s["over_ccap"] > 0
