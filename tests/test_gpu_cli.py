"""The command line on the GPU (readtape_amd/cli.py): cli.main in this process, one decode at a time, through the real front end, the device CSV parser and
the streaming reader - the labelled tape, the example command lines, -blklimit and -skip against what the reference wrote (tests/golden/cli_*.npz), a .csv
input against the converter route, --stream against the resident decode.  The cases are tests/cli_util.py's, shared with tests/test_cli_emul.py."""
import io
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cli_util as U
from readtape_amd import cli, csvin, csvout, pipeline

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["labelled_bin", "labelled_tap", "label_parity_bin"] + U.EXAMPLE_RUNS + U.OPTION_RUNS)
def test_command_lines_are_the_references(name, tmp_path):
    U.check_run(name, tmp_path, None)


def test_a_csv_input_is_parsed_on_the_device(tmp_path, monkeypatch):
    t = U.tape("nrzi9")
    hdr = t.spec.header()
    csvout.write_csv(str(tmp_path / "g.csv"), hdr, t.rows)
    seen = []
    real = csvin.read_csv_device
    monkeypatch.setattr(csvin, "read_csv_device", lambda *a, **k: seen.append(k) or real(*a, **k))
    assert cli.main(["-nrzi", "-nm", "-bpi=800", "-tap", "-nolabels", "-q", str(tmp_path / "g")], out=io.StringIO()) == 0
    assert len(seen) == 1 and seen[0]["ntrks"] == 9
    h2, rows, _ = csvin.read_csv(str(tmp_path / "g.csv"), ntrks=9, mode=hdr.mode, bpi=800.0, ips=50.0)
    ref = str(tmp_path / "ref.tap")
    pipeline.decode_tape(h2, rows, ref)
    mine = open(tmp_path / "g.tap", "rb").read()
    assert mine == open(ref, "rb").read() and len(mine) > 100


@pytest.mark.parametrize("extra", [[], ["-skip=700"]], ids=["plain", "skip"])
def test_stream_writes_the_resident_decodes_tap(extra, tmp_path):
    t = U.tape("nrzi9")
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    t.write(str(tmp_path / "a" / "g.tbin")), t.write(str(tmp_path / "b" / "g.tbin"))
    args = ["-nrzi", "-nm", "-tap", "-nolabels"] + extra
    assert cli.main(args + [str(tmp_path / "a" / "g")], out=io.StringIO()) == 0
    out = io.StringIO()
    assert cli.main(["--stream"] + args + [str(tmp_path / "b" / "g")], out=out) == 0
    assert out.getvalue().count("the streamed decode writes no log") == 1 and not os.path.exists(tmp_path / "b" / "g.log")
    resident = open(tmp_path / "a" / "g.tap", "rb").read()
    assert open(tmp_path / "b" / "g.tap", "rb").read() == resident and len(resident) > 100
    out = io.StringIO()
    assert cli.main(["--stream", "-q"] + args + [str(tmp_path / "b" / "g")], out=out) == 0
    assert out.getvalue() == f"{tmp_path}/b/g: ok\n"


def test_stream_is_refused_where_it_cannot_do_what_is_asked(tmp_path, capsys):
    U.tape("nrzi9").write(str(tmp_path / "g.tbin"))
    U.tape("ww").write(str(tmp_path / "w.tbin"))
    g, w = str(tmp_path / "g"), str(tmp_path / "w")
    for args, word in ((["--stream", "-nrzi", "-nolabels", g], "-tap"), (["--stream", "-whirlwind", "-tap", "-nolabels", w], "Whirlwind"),
                       (["--stream", "-nrzi", "-tap", "-nolabels", "-hex", g], "text file"), (["--stream", "-nrzi", "-tap", "-nolabels", "-blklimit=3", g], "-blklimit"),
                       (["--stream", "-nrzi", "-tap", g], "-nolabels")):
        assert cli.main(args, out=io.StringIO()) == 2, args
        assert word in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "g.tap")
