"""--peakstats / decode_tape(peakstats=True) on the GPU: cli.main in this process through the real front end - <base>.peakstats.csv, <base>.peakstats_deskew.csv
and the head-skew verdict against what the reference wrote for the same command lines (tests/golden/peakstats_*.npz), the statistics of the Python interface,
the option left out, the decodes that refuse it.  The cases are tests/peakstats_util.py's, shared with tests/test_emul_peakstats.py."""
import io
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peakstats_util as U
from readtape_amd import cli, ingest, pipeline, shard

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(U.RUNS))
def test_statistics_files_and_verdicts_are_the_references(name, tmp_path):
    U.check_run(name, tmp_path, None)


@pytest.mark.parametrize("name", ["ex_nrzi9", "skew_m_deskew"])
def test_the_statistics_of_the_python_interface(name, tmp_path):
    g = U.load(name)
    t = U.tape(g["tape"])
    base = str(tmp_path / "g")
    st, _ = pipeline.decode_tape(t.spec.header(), t.rows, None, log_path=base + ".log", opts=pipeline.DecodeOptions(multiple_tries=True), out_base=base,
                                 in_name="g.tbin", tap_format="-tap" in g["opts"], labels=True, deskew="-deskew" in g["opts"], peakstats=True)
    for key, f in (("peakstats", "g.peakstats.csv"), ("peakstats_deskew", "g.peakstats_deskew.csv")):
        assert (key in st) == (f in g["files"])
        if key in st:
            p = st[key]
            assert p["path"] == str(tmp_path / f) and open(p["path"], "rb").read() == g["files"][f]
            assert p["counts"].shape == (9, 50)
            assert list(p["counts"].sum(axis=1)) == [int(l.split(b",")[0]) for l in g["files"][f].splitlines()[1:]]
    assert st["skew_ok"] is (g["log"][-1] == U.SENTENCES[0] or g["log"][-1].endswith("successful"))
    st3, _ = pipeline.decode_tape(t.spec.header(), t.rows, str(tmp_path / "third.tap"))
    assert "peakstats" not in st3 and not os.path.exists(tmp_path / "third.peakstats.csv")


def test_attempts_read_from_exact_rescans_count_once(tmp_path):
    import cases
    t = U.tape("flood")
    st, _ = pipeline.decode_tape(t.spec.header(), t.rows, str(tmp_path / "g.tap"), find_zeros=True, differentiate=True, peakstats=True)
    assert st["exact_scans"] > 0 and st["skew_ok"] is False
    assert open(st["peakstats"]["path"], "rb").read() == U.load("flood")["files"]["g.peakstats.csv"]
    t = U.tape("nrzi7_restart")
    st, _ = pipeline.decode_tape(t.spec.header(), t.rows, str(tmp_path / "r.tap"), parms_text=cases.DESKEW_RESTART_PARMS, peakstats=True)
    assert st["exact_scans"] > 0
    assert open(st["peakstats"]["path"], "rb").read() == U.load("restart")["files"]["g.peakstats.csv"]


def test_nothing_of_it_without_the_option(tmp_path):
    status, console = U.run_cli("skew_m_deskew", str(tmp_path), None, extra=())
    assert status == 0
    assert not [f for f in os.listdir(tmp_path) if "peakstats" in f]
    assert not U.peak_lines(open(tmp_path / "g.log").read()) and not U.peak_lines(console)


def test_fragments_streams_and_shards_refuse_it(tmp_path, capsys):
    t = U.tape("nrzi9")
    hdr, rows = t.spec.header(), t.rows
    t.write(str(tmp_path / "g.tbin"))
    tap = str(tmp_path / "g.tap")
    calls = [lambda: pipeline.decode_tape_fragments(hdr, rows, tap, [(0, rows.shape[0])], peakstats=True),
             lambda: ingest.decode_file_streaming(str(tmp_path / "g.tbin"), tap, peakstats=True),
             lambda: shard.decode_sharded(hdr, rows, 0, rows.shape[0], 0, 1, None, tap, peakstats=True),
             lambda: shard.decode_file_sharded(str(tmp_path / "g.tbin"), tap, 0, 1, None, peakstats=True)]
    for call in calls:
        with pytest.raises(ValueError, match="peakstats"):
            call()
    assert cli.main(["--stream", "--peakstats", "-nrzi", "-tap", "-nolabels", str(tmp_path / "g")], out=io.StringIO()) == 2
    err = capsys.readouterr().err
    assert "--peakstats" in err and err.count("\n") == 1
    assert not os.path.exists(tap)
