"""The windowed decode with the kernels run by the CPU emulator: pipeline.decode_tape_windows - fragments that journal their blocks, one finisher that puts them
out - against the resident decode (pipeline.decode_tape) of the same tape with the same options: the same files byte for byte, the same log line by line,
the same statistics (tests/windows_util.py).  Every case with three span plans (one span; every block its own fragment; cuts inside blocks) and with the
fragments' replays on one thread and on three; the block limit in three positions; the peak statistics with the fragments replayed in reverse order."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import windows_util as U
from emul_util import emul_frontend
from readtape_amd import pipeline

_resident = {}


def resident(name, tmp_path_factory, **more):
    """the yardstick of a case, decoded once"""
    key = (name, tuple(sorted(more.items())))
    if key not in _resident:
        wd = str(tmp_path_factory.mktemp("resident"))
        _resident[key] = (wd, U.resident(name, wd, emul_frontend, **more))
    return _resident[key]


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("kind", U.PLANS)
@pytest.mark.parametrize("name", sorted(n for n in U.CASES if not n.endswith("_long") and n != "nrzi_weak_long_m"))      # (the long variants are the GPU tests')
def test_windows_put_out_what_the_resident_decode_does(name, kind, threads, tmp_path, tmp_path_factory):
    wd_a, st_a = resident(name, tmp_path_factory)
    t = U.tape(U.CASES[name][0])
    spans = U.plan(t, kind)
    assert len(spans) == {"one": 1}.get(kind, len(spans)) and (kind == "one" or len(spans) >= 2)
    st_b = U.windows(name, str(tmp_path), emul_frontend, spans, threads=threads)
    U.compare(wd_a, st_a, str(tmp_path), st_b, work="equal" if kind == "one" else U.work_sum(st_b["spans"]))
    assert sum(s["records"] for s in st_b["spans"]) >= st_b["blocks"] + st_b["tapemarks"]
    if kind == "gaps":                                        # every block (and tape mark) is its own fragment
        assert max(s["records"] for s in st_b["spans"]) == 1 and len(st_b["spans"]) == len(t.blocks)


def test_what_the_cases_are_about(tmp_path_factory):
    """the yardsticks themselves: label-named and numbered files, label lines, a block that needed more than one try, text files, both statistics files"""
    wd, st = resident("labelled_bin", tmp_path_factory)
    assert sorted(f for f in os.listdir(wd) if f.endswith(".bin")) == ["g-001-DOCUMENT.bin", "g-002-NOTES.bin"]
    assert any(l.startswith("*** tape label HDR1") for l in U.all_log_lines(wd))
    wd, st = resident("marks_bin", tmp_path_factory)
    assert {"g.001.bin", "g.002.bin", "g.003.bin"} <= set(os.listdir(wd))
    wd, st = resident("nrzi_weak_m", tmp_path_factory)
    log = U.all_log_lines(wd)
    tries = [int(m.group(1)) for m in (re.search(r", (\d+) tries, parmset", l) for l in log) if m]
    assert tries and max(tries) > 1, log
    good = [int(l.split()[0]) for l in log if l.endswith("good blocks had to try more than one parmset")]
    used = [l for l in log if re.match(r"  parmset \d+ was tried +\d+ times and used +\d+ times", l)]
    assert good and len(used) >= 2, log
    assert any(f.endswith(".txt") for f in os.listdir(resident("text_hex_ebcdic", tmp_path_factory)[0]))
    assert any(f.endswith(".txt") for f in os.listdir(resident("text_linefeed", tmp_path_factory)[0]))
    wd, st = resident("peaks_deskew", tmp_path_factory)
    assert sorted(U.peak_files(wd)) == ["g.peakstats.csv", "g.peakstats_deskew.csv"] and st["skew"] and "skew_ok" in st
    wd, st = resident("peaks_restart", tmp_path_factory)
    assert st["exact_scans"] > 0                              # an attempt restarted on an exact rescan: the histogram's roll-back, inside a fragment


U.CASES["marks_tap"] = ("labelled", dict(opts=U.NM, tap_format=True, labels=False))      # B B B M B B M B B M B B M B M B B M M: every block counts, no mark does
BLK = "marks_tap"


def _blk_plan():
    """three fragments: the first owns the tape's first three blocks, the second the mark behind them and three blocks"""
    t = U.tape("labelled")
    cut = lambda i: U.grid((t.blocks[i][2] + t.blocks[i + 1][1]) // 2)
    return [(0, cut(2)), (cut(2), cut(7)), (cut(7), int(t.rows.shape[0]))]


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("limit", [4, 3, 1000, 0])
def test_blklimit_inside_a_fragment_at_its_end_and_beyond_the_tape(limit, threads, tmp_path, tmp_path_factory):
    wd_a, st_a = resident(BLK, tmp_path_factory, blklimit=limit)
    st_b = U.windows(BLK, str(tmp_path), emul_frontend, _blk_plan(), blklimit=limit, threads=threads)
    U.compare(wd_a, st_a, str(tmp_path), st_b, work=None if limit < 1000 else U.work_sum(st_b["spans"]))      # (a limit inside a journal: that fragment's counters up to the block)
    if "whole" not in _resident:
        _resident["whole"] = U.windows(BLK, str(tmp_path_factory.mktemp("whole")), emul_frontend, _blk_plan())
    whole = _resident["whole"]
    assert [s["records"] for s in whole["spans"]][0] == 3     # the first fragment owns exactly three blocks: 3 ends it, 4 falls inside the second
    assert st_b["blocks"] == min(limit, whole["blocks"])
    assert ("***blklimit=%d reached" % limit in U.all_log_lines(str(tmp_path))) == (limit <= whole["blocks"])


@pytest.mark.parametrize("limit", [0, 2, 5, 1000])
def test_blklimit_in_one_span_counts_the_replays_work_as_the_resident_decode_does(limit, tmp_path, tmp_path_factory):
    """one fragment is the resident replay: the counters a record carries at the block limit, and the fragment's at its end, are the resident decode's"""
    wd_a, st_a = resident(BLK, tmp_path_factory, blklimit=limit)
    t = U.tape("labelled")
    st_b = U.windows(BLK, str(tmp_path), emul_frontend, U.plan(t, "one"), blklimit=limit)
    U.compare(wd_a, st_a, str(tmp_path), st_b, work="equal")


def test_blklimit_with_peak_statistics(tmp_path, tmp_path_factory):
    """the histogram is the one of the transitions up to the limiting block, which lies inside a journal"""
    wd_a, st_a = resident(BLK, tmp_path_factory, blklimit=4, peakstats=True)
    st_b = U.windows(BLK, str(tmp_path), emul_frontend, _blk_plan(), blklimit=4, peakstats=True, threads=3)
    U.compare(wd_a, st_a, str(tmp_path), st_b, work=None)


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("name", ["peaks", "peaks_restart"])
def test_the_bins_are_the_first_transitions_whichever_fragment_runs_first(name, threads, tmp_path, tmp_path_factory):
    wd_a, st_a = resident(name, tmp_path_factory)
    t = U.tape(U.CASES[name][0])
    st_b = U.windows(name, str(tmp_path), emul_frontend, U.plan(t, "gaps"), threads=threads, replay_order=lambda idx: list(reversed(idx)))
    U.compare(wd_a, st_a, str(tmp_path), st_b, work=U.work_sum(st_b["spans"]))
    assert len(st_b["spans"]) >= 3 and st_b["peakstats"]["binwidth"] > 0


def test_whirlwind_is_refused():
    t = U.tape("ww")
    with pytest.raises(NotImplementedError, match="Whirlwind"):
        pipeline.decode_tape_windows(t.spec.header(), t.rows, [(0, int(t.rows.shape[0]))], tap_path="x.tap", fe_factory=emul_frontend)

