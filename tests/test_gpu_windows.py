"""The windowed decode on the GPU: ingest.decode_file_windows and the command line's --windows - the streaming reader's pipeline with the journal and the
finisher behind it - against the resident decode of the same file with the same options (tests/windows_util.py: the same files byte for byte, the same log
line by line, the same statistics).  Windows and halos of 4096 rows, so every tape falls into four or more windows and blocks longer than a halo are met."""
import io
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cli_util
import windows_util as U
from readtape_amd import cli, ingest, pipeline

pytestmark = pytest.mark.gpu

_resident = {}
GPU_CASES = ["labelled_bin", "nrzi_weak_long_m", "pe_long", "gcr", "marks_bin", "text_hex_ebcdic", "text_linefeed_long", "peaks_long", "peaks_deskew"]      # (four windows and more each)


def resident(name, tmp_path_factory, **more):
    key = (name, tuple(sorted(more.items())))
    if key not in _resident:
        wd = str(tmp_path_factory.mktemp("resident"))
        _resident[key] = (wd, U.resident(name, wd, None, **more))
    return _resident[key]


def windows(name, wd, **more):
    """ingest.decode_file_windows on the case's tape written to <wd>/g.tbin, with decode_tape's arguments of the case"""
    tname, kw = U.CASES[name]
    kw = dict(kw, **more)
    U.tape(tname).write(os.path.join(wd, "g.tbin"))
    kw.setdefault("window_rows", 4096)
    kw.setdefault("halo_rows", 4096)
    return ingest.decode_file_windows(os.path.join(wd, "g.tbin"), out_base=os.path.join(wd, "g"), log_path=os.path.join(wd, "g.log"), in_name="g.tbin", **kw)


def fragment_work(st):
    """what the windowed decode's work counters are made of: the sum of its fragments' own replay statistics (tests/windows_util.py)"""
    return {k: st["fragment_work"][k] for k in U.WORK}


# (plan_windows ramps only windows of 2^20 rows and more: at 4096 rows `ramp` changes nothing and is not a parameter here; test_ramped_windows_of_unequal_size
#  below decodes a tiled tape through ramped windows)
@pytest.mark.parametrize("threads,split", [(1, 1), (3, 2)])
@pytest.mark.parametrize("name", GPU_CASES)
def test_a_streamed_file_gets_the_resident_decodes_outputs(name, threads, split, tmp_path, tmp_path_factory):
    wd_a, st_a = resident(name, tmp_path_factory)
    st_b = windows(name, str(tmp_path), replay_threads=threads, replay_split=split)
    assert st_b["windows"] >= 4 and st_b["windows_read"] == st_b["windows"]
    U.compare(wd_a, st_a, str(tmp_path), st_b, work=fragment_work(st_b))      # (every key, "bursts" - the windows' own, summed - included)
    assert st_b["finisher_seconds"] >= 0 and st_b["finisher_wait_seconds"] >= 0 and st_b["fragments"] >= 1


@pytest.mark.parametrize("limit", [None, 2])
@pytest.mark.parametrize("name", ["marks_bin", "nrzi_weak_long_m"])
def test_one_window_does_the_resident_replays_work(name, limit, tmp_path, tmp_path_factory):
    """a file that fits one window, one replay thread: one fragment from the first row to the last, whose replay is the resident decode's - the work
    counters too, at the block limit (a record's) and at the end (the fragment's)"""
    wd_a, st_a = resident(name, tmp_path_factory, blklimit=limit)
    st_b = windows(name, str(tmp_path), blklimit=limit, window_rows=1 << 16, halo_rows=4096)
    assert st_b["windows"] == 1 and st_b["fragments"] == 1
    U.compare(wd_a, st_a, str(tmp_path), st_b, work="equal")


def test_ramped_windows_of_unequal_size(tmp_path, tmp_path_factory):
    """ramp on, windows of 2^20 rows: the labelled tape tiled to 2.3 M rows goes as windows of 2^18, 2^19, 2^20 ... rows"""
    import numpy as np
    t = U.tape("labelled")
    U._tapes["labelled_x40"] = type(t)(spec=t.spec, rows=np.tile(t.rows, (40, 1)), blocks=[])
    U.CASES["tiled"] = ("labelled_x40", dict(opts=U.NM, tap_format=True, labels=True))
    assert len({hi - lo for lo, hi, _, _ in ingest.plan_windows(40 * t.rows.shape[0], 1 << 20, 1 << 17)}) >= 3
    wd_a, st_a = resident("tiled", tmp_path_factory)
    st_b = windows("tiled", str(tmp_path), window_rows=1 << 20, halo_rows=1 << 17, replay_threads=3, replay_split=2, ramp=True)
    assert st_b["windows"] >= 4
    U.compare(wd_a, st_a, str(tmp_path), st_b, work=fragment_work(st_b))


def test_the_weak_tape_needs_more_than_one_try(tmp_path_factory):
    wd, st = resident("nrzi_weak_long_m", tmp_path_factory)
    log = U.all_log_lines(wd)
    assert any(", 8 tries, parmset" in l for l in log) and sum("was tried" in l and "and used" in l for l in log) >= 2, log


def test_subsample_and_skip(tmp_path, tmp_path_factory):
    name = ("nrzi9_oversampled", dict(opts=U.NM, tap_format=True, labels=True))
    U.CASES["oversampled"] = name
    gap = cli_util._skips()[0]
    wd_a, st_a = resident("oversampled", tmp_path_factory, subsample=2, skip=gap)
    st_b = windows("oversampled", str(tmp_path), subsample=2, skip=gap, replay_threads=3, replay_split=2)
    U.compare(wd_a, st_a, str(tmp_path), st_b, work=fragment_work(st_b))
    assert st_b["windows"] >= 3                               # (10 000 used rows)


def _run(argv, wd, tname, parms=None):
    os.makedirs(wd, exist_ok=True)
    U.tape(tname).write(os.path.join(wd, "g.tbin"))
    if parms:
        open(os.path.join(wd, "g.parms"), "w").write(parms)
    out = io.StringIO()
    return cli.main(list(argv) + [os.path.join(wd, "g")], out=out), out.getvalue()


@pytest.mark.parametrize("run", ["labelled_bin", "labelled_tap", "ex_nrzi9", "ex_nrzi7", "ex_pe"])
def test_the_command_line_with_and_without_windows(run, tmp_path):
    tname, opts = cli_util.RUNS[run]
    a, b = str(tmp_path / "resident"), str(tmp_path / "windows")
    sa, ca = _run(opts, a, tname)
    sb, cb = _run(["--windows=4096"] + opts, b, tname)
    assert sa == 0 and sb == 0, (ca, cb)
    U.compare(a, None, b, None)
    console = lambda text, wd: [U.ELAPSED.sub("processed in 0 seconds (0.000 seconds/block)", l.rstrip()) for l in text.replace(wd + os.sep, "").splitlines()]
    assert console(ca, a) == console(cb, b)                   # the log is on the console too, exactly as on the resident path


def test_the_command_line_with_peakstats_and_deskew(tmp_path):
    opts = ["-v", "-m", "-nrzi", "-tap", "-deskew", "--peakstats"]
    a, b = str(tmp_path / "resident"), str(tmp_path / "windows")
    assert _run(opts, a, "nrzi9_skew_long")[0] == 0 and _run(["--windows=4096"] + opts, b, "nrzi9_skew_long")[0] == 0
    U.compare(a, None, b, None)
    assert sorted(U.peak_files(b)) == ["g.peakstats.csv", "g.peakstats_deskew.csv"]


def test_the_default_window_is_streams(tmp_path):
    a, b = str(tmp_path / "resident"), str(tmp_path / "windows")
    opts = cli_util.RUNS["labelled_bin"][1]
    assert _run(opts, a, "labelled")[0] == 0 and _run(["--windows"] + opts, b, "labelled")[0] == 0
    U.compare(a, None, b, None)


def test_the_three_refusals(tmp_path, capsys):
    wd = str(tmp_path)
    U.tape("nrzi9").write(os.path.join(wd, "g.tbin"))
    assert cli.main(["--windows", "--stream", "-nrzi", "-tap", "-nolabels", os.path.join(wd, "g")], out=io.StringIO()) == 2
    err = capsys.readouterr().err
    assert "--stream" in err and "--windows" in err and err.count("\n") == 1
    U.tape("ww").write(os.path.join(wd, "w.tbin"))
    assert cli.main(["--windows", "-whirlwind", "-tap", os.path.join(wd, "w")], out=io.StringIO()) == 2
    err = capsys.readouterr().err
    assert "Whirlwind" in err and err.count("\n") == 1
    open(os.path.join(wd, "c.csv"), "w").write("export\nTime [s], a, b, c, d, e, f, g, h, i\n0.0, 0, 0, 0, 0, 0, 0, 0, 0, 0\n")
    assert cli.main(["--windows", "-nrzi", "-tap", os.path.join(wd, "c")], out=io.StringIO()) == 2
    err = capsys.readouterr().err
    assert ".tbin" in err and err.count("\n") == 1
    assert sorted(os.listdir(wd)) == ["c.csv", "g.tbin", "w.tbin"]
    assert "--windows" in cli.USAGE


def test_blklimit_stops_the_reads(tmp_path, tmp_path_factory):
    U.CASES["marks_tap"] = ("labelled", dict(opts=U.NM, tap_format=True, labels=False))
    wd_a, st_a = resident("marks_tap", tmp_path_factory, blklimit=2)
    st_b = windows("marks_tap", str(tmp_path), blklimit=2, replay_threads=3, replay_split=2, scan_contexts=2)
    # (the reads stop: "bursts" counts the windows that were decoded, not the tape's; the limit falls inside a journal: tests/windows_util.py on work=None)
    U.compare(wd_a, {k: v for k, v in st_a.items() if k != "bursts"}, str(tmp_path), st_b, work=None)
    assert st_b["blocks"] == 2 and st_b["windows"] >= 12 and st_b["windows_read"] < st_b["windows"] and st_b["bursts"] < st_a["bursts"]
    a, b = str(tmp_path / "resident"), str(tmp_path / "windows")
    opts = ["-v", "-nm", "-nrzi", "-tap", "-blklimit=1"]
    assert _run(opts, a, "labelled")[0] == 0 and _run(["--windows=4096"] + opts, b, "labelled")[0] == 0
    U.compare(a, None, b, None)                               # (the command line hands no statistics back: its decode is the call above with its options)
