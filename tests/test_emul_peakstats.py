"""--peakstats / decode_tape(peakstats=True) with the kernels run by the CPU emulator: <base>.peakstats.csv, <base>.peakstats_deskew.csv and the head-skew
verdict against what the reference wrote for the same command lines (tests/golden/peakstats_*.npz, tests/make_peakstats_golden.py) - the files byte for byte,
the log lines in order, everything else as without the option -, the statistics of the Python interface, the option left out, the decodes that refuse it, the
help text.  The cases are tests/peakstats_util.py's, shared with tests/test_gpu_peakstats.py."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peakstats_util as U
from emul_util import emul_frontend
from readtape_amd import cli, ingest, pipeline, shard


@pytest.mark.parametrize("name", sorted(U.RUNS))
def test_statistics_files_and_verdicts_are_the_references(name, tmp_path):
    U.check_run(name, tmp_path, emul_frontend)


def test_what_the_goldens_are_about():
    """the goldens themselves: every try counts, both catch-all bins fill, the two files of a skewed tape differ, -q keeps only the pre-pass' file"""
    total = lambda name, f="g.peakstats.csv": sum(int(l.split(b",")[0]) for l in U.load(name)["files"][f].splitlines()[1:])
    ends = lambda name, f="g.peakstats.csv": [sum(int(l.split(b",")[k]) for l in U.load(name)["files"][f].splitlines()[1:]) for k in (1, 2)]
    assert total("weak_m") > 5 * total("weak_nm") and min(ends("weak_m")) > 0
    assert ends("skew_long", "g.peakstats_deskew.csv")[1] > 1000 and ends("pe_drop")[0] > 0
    for name in ("ww_skew", "skew_m_deskew", "skew_long", "nobpi_skew"):
        f = U.load(name)["files"]
        assert sorted(f) == ["g.peakstats.csv", "g.peakstats_deskew.csv"] and f["g.peakstats.csv"] != f["g.peakstats_deskew.csv"]
    assert sorted(U.load("quiet")["files"]) == ["g.peakstats_deskew.csv"] and not U.load("quiet")["log"]
    assert total("noise") == 0 and b"nan" in U.load("noise")["files"]["g.peakstats.csv"]
    assert U.load("skew_m_deskew")["log"][-1].endswith("seems to have been successful")
    assert U.load("gcr_skew")["log"][-3].endswith("wasn't entirely effective")
    assert U.load("ex_nrzi9")["log"][-1] == U.SENTENCES[0] and U.load("ex_pe")["log"][-1] == U.load("ex_gcr")["log"][-1] == U.SENTENCES[1]


def _file_totals(data):
    return [int(l.split(b",")[0]) for l in data.splitlines()[1:]]


@pytest.mark.parametrize("name", ["ex_nrzi9", "skew_m_deskew"])
def test_the_statistics_of_the_python_interface(name, tmp_path):
    g = U.load(name)
    t = U.tape(g["tape"])
    deskew = "-deskew" in g["opts"]
    base = str(tmp_path / "g")
    st, _ = pipeline.decode_tape(t.spec.header(), t.rows, None, log_path=base + ".log", opts=pipeline.DecodeOptions(multiple_tries=True), fe_factory=emul_frontend,
                                 out_base=base, in_name="g.tbin", tap_format="-tap" in g["opts"], labels=True, deskew=deskew, peakstats=True)
    for key, f in (("peakstats", "g.peakstats.csv"), ("peakstats_deskew", "g.peakstats_deskew.csv")):
        assert (key in st) == (f in g["files"])
        if key not in st:
            continue
        p = st[key]
        assert p["path"] == str(tmp_path / f) and open(p["path"], "rb").read() == g["files"][f]
        assert p["counts"].shape == (9, 50) and p["counts"].dtype.kind == "i" and p["binwidth"] > 0
        assert list(p["counts"].sum(axis=1)) == _file_totals(g["files"][f])
        assert list(p["trksums"]) == list(p["counts"][:, 1:49].sum(axis=1))
    assert st["skew_ok"] is (g["log"][-1] == U.SENTENCES[0] or g["log"][-1].endswith("successful"))
    assert 0 <= st["skew_peak_frac"] < 0.2 and 0 <= st["skew_stddev_frac"] < 0.05
    line = [l for l in g["log"] if l.startswith("  that peak difference")][-1]
    pct = lambda x: float(np.float32(x) * np.float32(100))                     # (the log's product is a float's)
    assert f"are {pct(st['skew_peak_frac']):.1f}% and {pct(st['skew_stddev_frac']):.1f}%" in line
    # a tap_path names the files too, and the next decode on this thread gathers nothing
    st2, _ = pipeline.decode_tape(t.spec.header(), t.rows, str(tmp_path / "other.tap"), fe_factory=emul_frontend, peakstats=True)
    assert st2["peakstats"]["path"] == str(tmp_path / "other.peakstats.csv") and os.path.exists(st2["peakstats"]["path"])
    st3, _ = pipeline.decode_tape(t.spec.header(), t.rows, str(tmp_path / "third.tap"), fe_factory=emul_frontend)
    assert "peakstats" not in st3 and "skew_ok" not in st3 and not os.path.exists(tmp_path / "third.peakstats.csv")


def test_attempts_read_from_exact_rescans_count_once(tmp_path):
    """the flood tape is decoded from an exact rescan; the restart tape's first attempt is started on the burst table, crosses a device restart with state
    and is replayed from its first row on an exact rescan: their transitions are in the histogram once (the goldens' files are the reference's, which reads
    every attempt once)"""
    import cases
    g = U.load("flood")
    t = U.tape("flood")
    st, _ = pipeline.decode_tape(t.spec.header(), t.rows, str(tmp_path / "g.tap"), fe_factory=emul_frontend, find_zeros=True, differentiate=True, peakstats=True)
    assert st["exact_scans"] > 0
    assert open(st["peakstats"]["path"], "rb").read() == g["files"]["g.peakstats.csv"]
    assert st["skew_ok"] is False
    g = U.load("restart")
    t = U.tape("nrzi7_restart")
    st, _ = pipeline.decode_tape(t.spec.header(), t.rows, str(tmp_path / "r.tap"), fe_factory=emul_frontend, parms_text=cases.DESKEW_RESTART_PARMS, peakstats=True)
    assert st["exact_scans"] > 0
    assert open(st["peakstats"]["path"], "rb").read() == g["files"]["g.peakstats.csv"]


def test_nothing_of_it_without_the_option(tmp_path):
    status, console = U.run_cli("skew_m_deskew", str(tmp_path), emul_frontend, extra=())
    assert status == 0
    assert not [f for f in os.listdir(tmp_path) if "peakstats" in f]
    log = open(tmp_path / "g.log").read()
    assert not U.peak_lines(log) and not U.peak_lines(console) and "statistics file" not in log and "earliest peak" not in log


def test_a_list_gives_every_file_its_own_statistics(tmp_path):
    U.tape("nrzi9").write(str(tmp_path / "a.tbin"))
    U.tape("nrzi9_skew").write(str(tmp_path / "b.tbin"))
    (tmp_path / "list.txt").write_text(f"{tmp_path}/a\n{tmp_path}/b\n")
    assert cli.main(["-nrzi", "-m", "-tap", "-v", "--peakstats", "-f", str(tmp_path / "list")], fe_factory=emul_frontend, out=io.StringIO()) == 0
    b = open(tmp_path / "b.peakstats.csv", "rb").read()
    assert b == U.load("skew_m")["files"]["g.peakstats.csv"] and open(tmp_path / "a.peakstats.csv", "rb").read() != b
    assert [l.replace("b.peakstats", "g.peakstats") for l in U.peak_lines(open(tmp_path / "b.log").read().replace(str(tmp_path) + os.sep, ""))] == U.load("skew_m")["log"]


def test_fragments_streams_and_shards_refuse_it(tmp_path):
    t = U.tape("nrzi9")
    hdr, rows = t.spec.header(), t.rows
    t.write(str(tmp_path / "g.tbin"))
    tap = str(tmp_path / "g.tap")
    calls = [lambda: pipeline.decode_tape_fragments(hdr, rows, tap, [(0, rows.shape[0])], fe_factory=emul_frontend, peakstats=True),
             lambda: pipeline.decode_fragment(hdr, None, None, None, rows, 0, 0, None, tap, [], None, peakstats=True),
             lambda: pipeline.decode_fragments(hdr, None, None, None, rows, 0, [0], [None], [tap], [], None, peakstats=True),
             lambda: ingest.decode_file_streaming(str(tmp_path / "g.tbin"), tap, peakstats=True),
             lambda: shard.decode_sharded(hdr, rows, 0, rows.shape[0], 0, 1, None, tap, peakstats=True),
             lambda: shard.decode_file_sharded(str(tmp_path / "g.tbin"), tap, 0, 1, None, peakstats=True)]
    for call in calls:
        with pytest.raises(ValueError, match="peakstats"):
            call()
    assert not os.path.exists(tap) and not [f for f in os.listdir(tmp_path) if "peakstats" in f]


def test_stream_refuses_it_with_status_2_and_one_line(tmp_path, capsys):
    U.tape("nrzi9").write(str(tmp_path / "g.tbin"))
    assert cli.main(["--stream", "--peakstats", "-nrzi", "-tap", "-nolabels", str(tmp_path / "g")], fe_factory=emul_frontend, out=io.StringIO()) == 2
    err = capsys.readouterr().err
    assert "--peakstats" in err and err.count("\n") == 1
    assert not os.path.exists(tmp_path / "g.tap")


def test_the_help_text_explains_it():
    assert "--peakstats" in cli.USAGE and "peakstats.csv is not written" in cli.USAGE
    for refused in ("-showibg=n", "-sumt=sss", "-sumc=ccc", "-adjskew", "-d[n]"):
        assert refused in cli.USAGE.split("not built")[1]
    assert np.all([cli.main([o, "x"], out=io.StringIO()) == 2 for o in ("-showibg=3", "-sumt=s", "-sumc=c", "-adjskew", "-d")])
