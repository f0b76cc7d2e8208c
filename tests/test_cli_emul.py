"""The command line end to end (readtape_amd/cli.py) with the kernels run by the CPU emulator: the labelled tapes and the example command lines against what the
reference wrote for them (tests/golden/cli_*.npz, tests/make_cli_golden.py) - file names, file bytes, log lines -, -blklimit and -skip, -q, a list run,
-tapread, a .csv input, and `python -m readtape_amd` as a child process.  The cases are tests/cli_util.py's, shared with tests/test_gpu_cli.py."""
import io
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cli_util as U
import textfile_util
from emul_util import emul_frontend
from readtape_amd import cli, csvin, csvout, pipeline, textfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", U.LABEL_RUNS)
def test_labelled_tapes_are_the_references(name, tmp_path):
    console, log = U.check_run(name, tmp_path, emul_frontend)
    assert U.label_lines(console) == U.label_lines(log)                      # (not quiet: the log's text is on the console too)


def test_what_the_label_variants_are_about():
    """the goldens themselves: a flipped H and an 81st byte make a numbered file, a parity error leaves a label a label"""
    assert sorted(U.load("labelled_bin")["files"]) == ["g-001-DOCUMENT.bin", "g-002-NOTES.bin"]
    assert "g-002-SECOND.bin" in U.load("label_parity_bin")["files"] and "--> 1 errors" in U.load("label_parity_bin")["log"]
    for name in ("flipped_h_bin", "81_bytes_bin"):
        g = U.load(name)
        assert "g.002.bin" in g["files"] and not any("SECOND" in f for f in g["files"])
        assert len(g["files"]["g.002.bin"]) == (81 if name == "81_bytes_bin" else 80)
    assert not U.label_lines("\n".join(U.load("labelled_nolabels")["log"]))
    assert sum(l.startswith("*** tape label") for l in U.load("labelled_tap")["log"]) == 9


def test_labels_are_off_unless_asked_for(tmp_path):
    """pipeline.decode_tape(labels=False), the default: the files of -nolabels"""
    g = U.load("labelled_nolabels")
    t = U.tape("labelled")
    base = str(tmp_path / "g")
    pipeline.decode_tape(t.spec.header(), t.rows, None, log_path=base + ".log", fe_factory=emul_frontend, out_base=base, in_name="g.tbin", tap_format=False)
    assert U.output_files(str(tmp_path)) == g["files"]
    st, _ = pipeline.decode_tape(t.spec.header(), t.rows, None, log_path=base + ".log", fe_factory=emul_frontend, out_base=base, in_name="g.tbin", tap_format=False,
                                 labels=True)
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("g-")) == ["g-001-DOCUMENT.bin", "g-002-NOTES.bin"] and st["blocks"] == 3


@pytest.mark.parametrize("name", U.EXAMPLE_RUNS + U.OPTION_RUNS)
def test_command_lines_are_the_references(name, tmp_path):
    U.check_run(name, tmp_path, emul_frontend)


def test_blklimit_and_skip_reach_the_decode(tmp_path):
    """what the goldens of -blklimit and -skip hold differs from the plain run's, so the options are not lost on the way"""
    records = lambda name: int((textfile.read_tap(U.load(name)["files"]["g.tap"])["kind"] == textfile.RECORD).sum())
    assert records("blklimit1") == 1 and records("skip_gap") == 2
    assert "***blklimit=1 reached" in U.load("blklimit1")["log"]
    taps = {n: U.load(n)["files"]["g.tap"] for n in ("skip_gap", "skip_block")}
    assert taps["skip_gap"] != taps["skip_block"]
    with pytest.raises(pipeline.ReferenceFatal):
        t = U.tape("nrzi9")
        pipeline.decode_tape(t.spec.header(), t.rows, str(tmp_path / "x.tap"), fe_factory=emul_frontend, skip=t.rows.shape[0] + 1)


def test_quiet_says_ok_or_bad_and_nothing_else(tmp_path):
    status, console = U.run_cli("skip_gap", str(tmp_path), emul_frontend, extra=["-q"])
    assert status == 0 and console == f"{tmp_path}/g: ok\n"
    status, console = U.run_cli("label_parity_tap", str(tmp_path), emul_frontend, extra=["-q"])      # (a block with a parity error)
    assert status == 0 and console == f"{tmp_path}/g: bad\n"


def test_quiet_in_the_directory_of_the_tape(tmp_path, monkeypatch):
    U.tape("nrzi9").write(str(tmp_path / "g.tbin"))
    monkeypatch.chdir(tmp_path)
    out = io.StringIO()
    assert cli.main(["-nrzi", "-nm", "-tap", "-q", "g"], fe_factory=emul_frontend, out=out) == 0
    assert out.getvalue() == "g: ok\n"


def test_nolog_writes_to_the_console_only(tmp_path):
    status, console = U.run_cli("labelled_bin", str(tmp_path), emul_frontend, extra=["-nolog"])
    assert status == 0 and not os.path.exists(tmp_path / "g.log")
    assert [l.replace(str(tmp_path) + os.sep, "") for l in U.log_lines(console)] == U.load("labelled_bin")["log"]


def test_a_list_of_two_tapes(tmp_path):
    """-f: one file per line, the options in front of a name stay in force; every file gets its ok / bad line"""
    U.tape("nrzi9").write(str(tmp_path / "a.tbin"))
    U.tape("nrzi7_order").write(str(tmp_path / "b.tbin"))
    (tmp_path / "list.txt").write_text(f"{tmp_path}/a\n\n-nm -ntrks=7 -order=543210p {tmp_path}/b.tbin\n")
    out = io.StringIO()
    assert cli.main(["-nrzi", "-tap", "-v", "-f", str(tmp_path / "list")], fe_factory=emul_frontend, out=out) == 0
    oks = [l for l in out.getvalue().splitlines() if l.endswith(": ok") or l.endswith(": bad")]
    assert oks == [f"{tmp_path}/a: ok", f"{tmp_path}/b.tbin: ok"]
    assert "good blocks had to try more than one parmset" in open(tmp_path / "a.log").read()       # -m was the default for the first ...
    assert "good blocks had to try more than one parmset" not in open(tmp_path / "b.log").read()   # ... and -nm held for the second
    assert open(tmp_path / "b.tap", "rb").read() == U.load("ex_nrzi7")["files"]["g.tap"]
    (tmp_path / "list2.txt").write_text(f"{tmp_path}/a\n{tmp_path}/missing\n{tmp_path}/b\n")
    os.remove(tmp_path / "b.tap")
    assert cli.main(["-nrzi", "-tap", "-f", str(tmp_path / "list2")], fe_factory=emul_frontend, out=io.StringIO()) == 99      # the list ends where the reference exits
    assert not os.path.exists(tmp_path / "b.tap")


def test_outf_and_outp(tmp_path):
    U.tape("nrzi9").write(str(tmp_path / "g.tbin"))
    (tmp_path / "res").mkdir()
    assert cli.main(["-nrzi", "-nm", "-tap", "-q", f"-outf={tmp_path}/res/named", str(tmp_path / "g")], fe_factory=emul_frontend, out=io.StringIO()) == 0
    assert sorted(os.listdir(tmp_path / "res")) == ["named.log", "named.tap"]


def test_parms_file_beside_the_tape(tmp_path):
    """<base>.parms is handed to the decode, and its readtape line is an option of the run"""
    t = U.tape("nrzi9")
    t.write(str(tmp_path / "g.tbin"))
    import cases
    (tmp_path / "g.parms").write_text("readtape -tap\n" + cases.DESKEW_RESTART_PARMS)
    out = io.StringIO()
    assert cli.main(["-nrzi", "-nm", "-v", "-nolabels", str(tmp_path / "g")], fe_factory=emul_frontend, out=out) == 0
    assert "reading parmsets from file" in out.getvalue()
    ref = str(tmp_path / "ref.tap")
    pipeline.decode_tape(t.spec.header(), t.rows, ref, fe_factory=emul_frontend, parms_text=cases.DESKEW_RESTART_PARMS)
    assert open(tmp_path / "g.tap", "rb").read() == open(ref, "rb").read()


def test_tapread_is_write_text(tmp_path):
    image = U.load("labelled_tap")["files"]["g.tap"]
    (tmp_path / "g.tap").write_bytes(image)
    out = io.StringIO()
    assert cli.main(["-tapread", "-hex", "-ebcdic", str(tmp_path / "g")], fe_factory=emul_frontend, out=out) == 0
    (tmp_path / "ref").mkdir()
    r = textfile.write_text(image, str(tmp_path / "ref" / "g"), textfile.TextOptions(num="hex", char="ebcdic"))
    mine = open(tmp_path / "g.hex.EBCDIC.txt", "rb").read()
    cut = lambda b: textfile_util.cut_date(b)[0].split(b"\n", 1)[1]           # (without the title's two lines: the file's own name, the date)
    assert cut(mine) == cut(open(r["name"], "rb").read()) and b"VOL1TAPE01" in mine
    assert cli.main(["-octal", str(tmp_path / "g.tap")], fe_factory=emul_frontend, out=io.StringIO()) == 0      # (the extension alone asks for it)
    assert os.path.exists(tmp_path / "g.octal.txt")
    (tmp_path / "cut.tap").write_bytes(image[:7] + b"\xff")
    assert cli.main(["-tapread", "-hex", str(tmp_path / "cut")], fe_factory=emul_frontend, out=io.StringIO()) == 99


def test_a_csv_input_goes_through_the_converter(tmp_path):
    t = U.tape("nrzi9")
    hdr = t.spec.header()
    csvout.write_csv(str(tmp_path / "g.csv"), hdr, t.rows)
    assert cli.main(["-nrzi", "-nm", "-bpi=800", "-tap", "-nolabels", "-q", str(tmp_path / "g")], fe_factory=emul_frontend, out=io.StringIO()) == 0
    h2, rows, _ = csvin.read_csv(str(tmp_path / "g.csv"), ntrks=9, mode=hdr.mode, bpi=800.0, ips=50.0)
    ref = str(tmp_path / "ref.tap")
    pipeline.decode_tape(h2, rows, ref, fe_factory=emul_frontend)
    mine = open(tmp_path / "g.tap", "rb").read()
    assert mine == open(ref, "rb").read() and len(mine) > 100
    t.write(str(tmp_path / "g.tbin"))                                          # with both, the .csv is found first unless -tbin says otherwise
    out = io.StringIO()
    assert cli.main(["-nrzi", "-nm", "-tap", "-tbin", str(tmp_path / "g")], fe_factory=emul_frontend, out=out) == 0
    assert f'reading file "{tmp_path}/g.tbin"' in out.getvalue()


def test_stream_is_refused_where_it_cannot_do_what_is_asked(tmp_path, capsys):
    U.tape("nrzi9").write(str(tmp_path / "g.tbin"))
    U.tape("ww").write(str(tmp_path / "w.tbin"))
    g, w = str(tmp_path / "g"), str(tmp_path / "w")
    for args, word in ((["--stream", "-nrzi", "-nolabels", g], "-tap"), (["--stream", "-whirlwind", "-tap", "-nolabels", w], "Whirlwind"),
                       (["--stream", "-nrzi", "-tap", "-nolabels", "-hex", g], "text file"), (["--stream", "-nrzi", "-tap", "-nolabels", "-blklimit=3", g], "-blklimit"),
                       (["--stream", "-nrzi", "-tap", g], "-nolabels")):
        assert cli.main(args, fe_factory=emul_frontend, out=io.StringIO()) == 2, args
        err = capsys.readouterr().err
        assert word in err and err.count("\n") == 1
    assert not os.path.exists(tmp_path / "g.tap")


def test_python_m_readtape_amd(tmp_path):
    (tmp_path / "g.tap").write_bytes(U.load("labelled_tap")["files"]["g.tap"])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "readtape_amd", "-tapread", "-hex", "-ebcdic", "g"], cwd=tmp_path, env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "processing g.tap" in p.stdout and os.path.getsize(tmp_path / "g.hex.EBCDIC.txt") > 1000
    p = subprocess.run([sys.executable, "-m", "readtape_amd", "-tapx", "g"], cwd=tmp_path, env=env, capture_output=True, text=True)
    assert p.returncode == 99 and p.stderr == "bad option: -tapx\n"


def test_a_header_that_knows_its_mode_wins_and_one_that_does_not_takes_the_options(tmp_path):
    import dataclasses
    t = U.tape("nrzi9")
    for sub, mode, opt in (("a", t.spec.mode, "-pe"), ("b", 0, "-nrzi")):
        (tmp_path / sub).mkdir()
        dataclasses.replace(t, spec=dataclasses.replace(t.spec, mode=mode)).write(str(tmp_path / sub / "g.tbin"))
        assert cli.main([opt, "-nm", "-tap", "-nolabels", "-q", str(tmp_path / sub / "g")], fe_factory=emul_frontend, out=io.StringIO()) == 0
    ref = str(tmp_path / "ref.tap")
    pipeline.decode_tape(t.spec.header(), t.rows, ref, fe_factory=emul_frontend)
    assert open(tmp_path / "a" / "g.tap", "rb").read() == open(tmp_path / "b" / "g.tap", "rb").read() == open(ref, "rb").read()
