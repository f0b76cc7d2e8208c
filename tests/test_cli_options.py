"""The command line's option grammar (readtape_amd/cli.py; the reference's, src/readtape.c:816-1033): keywords in any letter case and as the whole
argument, the four number bases, every range at its edges, the options whose order matters, the text options, the exit statuses with their messages, and
the parameter-set files.  No device and no native library: nothing here decodes."""
import io
import os

import pytest

from readtape_amd import cli, tbin

INT_MAX = 0x7fffffff


def parse(*args):
    return cli.parse_args(list(args))


def status_of(*args, capsys=None):
    return cli.main(list(args), out=io.StringIO())


# ---- matching ----
@pytest.mark.parametrize("arg, name, value", [
    ("-tap", "tap_format", True), ("-TAP", "tap_format", True), ("-Tap", "tap_format", True), ("-NoLabels", "labels", False), ("-ZEROS", "find_zeros", True),
    ("-fluxdir=AUTO", "fluxdir", "auto"), ("-FLUXDIR=pos", "fluxdir", "pos"), ("-Ebcdic", "char", "ebcdic"), ("-HEX", "num", "hex"), ("-sdsm", "char", "sdsm"),
    ("-SDS", "char", "sds"), ("-adagetape", "char", "adagetape"), ("-adage", "char", "adage"), ("-NTRKS=7", "ntrks_specified", 7), ("-OutF=x/Y", "outf", "x/Y"),
    ("-outp=Results/", "outp", "Results/"), ("-Q", "quiet", True), ("-F", "filelist", True), ("-nm", "multiple_tries", False), ("-nocorrect", "correct", False),
    ("--stream", "stream", True)])
def test_keywords_match_in_any_case(arg, name, value):
    o, rest = parse(arg, "g")
    assert getattr(o, name) == value and rest == ["g"]


@pytest.mark.parametrize("arg", ["-tapx", "-ta", "-tap=1", "-nrzi9", "-fluxdir=up", "-fluxdir=", "-hexa", "-octal3", "-v=3", "-vx", "-x", "-qq", "-ntrks", "-ntrks=",
                                 "-ntrks=7x", "-skip=1.5", "-bpi=8oo", "-ips=", "-linesize=0x", "-skip=0b102", "-skip=09", "-", "-order=01234567", "-order=0123456pp"])
def test_a_keyword_must_be_the_whole_argument(arg, capsys):
    assert status_of(arg, "g") == 99
    assert capsys.readouterr().err == f"bad option: {arg}\n"


@pytest.mark.parametrize("text, n", [("123", 123), ("0", 0), ("0x1F", 31), ("0X1f", 31), ("0b1010", 10), ("0B11", 3), ("0b", 0), ("017", 15), ("010", 8), ("00", 0)])
def test_the_four_number_bases(text, n):
    assert cli.parse_int(text) == n
    assert parse(f"-skip={text}")[0].skip == n


# ---- ranges: (option, first value inside, last value inside, attribute); one outside on either side is a bad option ----
RANGES = [("ntrks", 5, 19, "ntrks_specified"), ("skip", 0, INT_MAX, "skip"), ("blklimit", 0, INT_MAX, "blklimit"), ("revparity", 0, INT_MAX, "revparity"),
          ("subsample", 1, INT_MAX, "subsample"), ("linesize", 4, 400, "linesize"), ("dataspace", 0, 400, "dataspace")]


@pytest.mark.parametrize("opt, lo, hi, name", RANGES)
def test_integer_ranges(opt, lo, hi, name, capsys):
    for n in (lo, hi):
        assert getattr(parse(f"-{opt}={n}")[0], name) == n
    for n in (lo - 1, hi + 1):
        assert status_of(f"-{opt}={n}", "g") == 99
        assert capsys.readouterr().err == f"bad option: -{opt}={n}\n"


@pytest.mark.parametrize("opt, lo, hi, name", [("bpi", 100, 10000, "bpi_specified"), ("ips", 10, 200, "ips_specified")])
def test_float_ranges(opt, lo, hi, name):
    for x in (lo, hi, lo + 0.5):
        assert getattr(parse(f"-{opt}={x}")[0], name) == x
    for x in (lo - 1, hi + 1):
        assert status_of(f"-{opt}={x}", "g") == 99


def test_verbose_levels():
    assert parse("-v")[0].verbose and parse("-v")[0].verbose_level == 1
    for n in (0, 3, 255):
        o = parse(f"-v{n}")[0]
        assert o.verbose and o.verbose_level == n
    assert status_of("-v256", "g") == 99
    o = parse("-q", "-v")[0]
    assert o.verbose and not o.quiet
    o = parse("-v", "-q")[0]
    assert o.quiet and not o.verbose


def test_options_end_at_the_first_argument_without_a_dash():
    o, rest = parse("-tap", "g", "-nrzi")
    assert o.tap_format and o.mode == tbin.MODE_PE and rest == ["g", "-nrzi"]


# ---- order ----
def test_whirlwind_turns_multiple_tries_off_and_a_later_m_is_fatal(tmp_path, capsys):
    assert parse("-whirlwind")[0].multiple_tries is False and parse("-whirlwind")[0].bpi == 100.0
    assert parse("-m", "-whirlwind")[0].multiple_tries is False
    assert parse("-whirlwind", "-m")[0].multiple_tries is True
    assert status_of("-whirlwind", "-m", str(tmp_path / "g")) == 99
    assert "multiple decoding tries is not implemented yet for Whirlwind" in capsys.readouterr().err


def test_gcr_sets_the_speed_and_ips_wins_in_either_order():
    assert parse("-gcr")[0].resolved_ips() == 25.0
    assert parse("-gcr")[0].resolved_ips(header_ips=125.0) == 125.0           # (the header's speed wins over -gcr's)
    for args in (("-gcr", "-ips=50"), ("-ips=50", "-gcr")):
        o = parse(*args)[0]
        assert o.ips == 25.0 and o.ips_specified == 50.0 and o.resolved_ips() == 50.0 and o.resolved_ips(header_ips=125.0) == 50.0
    assert parse("-nrzi")[0].resolved_ips() == 50.0
    assert parse("-gcr", "-bpi=6250")[0].resolved_bpi(tbin.MODE_GCR) == 9042.0
    assert parse("-bpi=556")[0].resolved_bpi(tbin.MODE_NRZI, header_bpi=800.0) == 556.0
    assert parse("-nrzi")[0].resolved_bpi(tbin.MODE_NRZI, header_bpi=800.0) == 800.0
    assert parse("-whirlwind")[0].resolved_bpi(tbin.MODE_WW) == 100.0


def test_octal2_and_dataspace_in_either_order():
    assert parse("-octal2", "-dataspace=0")[0].dataspace == 0
    assert parse("-dataspace=0", "-octal2")[0].dataspace == 2
    assert parse("-octal2")[0].text_options().dataspace == 2
    assert parse("-octal")[0].text_options().dataspace == 0


def test_skew_needs_ntrks_in_front_of_it(capsys):
    assert status_of("-skew=1,2,3,4,5,6,7", "-ntrks=7", "g") == 99
    assert "must specify ntrks= to use skew=" in capsys.readouterr().err
    o = parse("-ntrks=7", "-skew=1,2,3,4,5,6,7")[0]
    assert o.skew == [1, 2, 3, 4, 5, 6, 7] and o.deskew
    for bad in ("-skew=1,2,3,4,5,6", "-skew=1,2,3,4,5,6,7,8", "-skew=1,2,3,4,5,6,x", "-skew=1 2 3 4 5 6 7"):
        assert status_of("-ntrks=7", bad, "g") == 99


def test_order_is_a_whirlwind_string_only_behind_whirlwind(capsys):
    o = parse("-whirlwind", "-order=CxMLcmxl")[0]
    assert o.order == "CxMLcmxl" and o.order_is_ww and o.ntrks == 6
    assert status_of("-order=CMLcml", "-whirlwind", "g") == 99
    assert capsys.readouterr().err == "bad option: -order=CMLcml\n"
    o = parse("-order=543210p")[0]
    assert o.order == "543210p" and not o.order_is_ww and o.ntrks == 7
    assert status_of("-whirlwind", "-order=CMLcmq", "g") == 99
    assert "bad Whirlwind track order symbol" in capsys.readouterr().err
    assert status_of("-whirlwind", "-order=CMxxxx", "g") == 99
    assert "primary LSB track" in capsys.readouterr().err
    assert status_of("-order=0123", "g") == 99
    assert "-order can't imply ntrks=4" in capsys.readouterr().err


# ---- text options ----
@pytest.mark.parametrize("args, expect", [
    ((), None), (("-textfile",), (None, None, 64)), (("-hex",), ("hex", None, 64)), (("-ascii",), (None, "ascii", 64)), (("-hex", "-ascii"), ("hex", "ascii", 32)),
    (("-octal2", "-flexo"), ("octal2", "flexo", 32)), (("-SDS", "-linesize=144"), (None, "sds", 144)), (("-hex", "-ebcdic", "-linesize=40"), ("hex", "ebcdic", 40)),
    (("-linesize=40",), None), (("-linefeed",), None)])
def test_a_type_implies_the_text_file_and_sets_the_line_size(args, expect):
    t = parse(*args)[0].text_options()
    assert (t if t is None else (t.num, t.char, t.linesize)) == expect


# ---- statuses ----
def test_statuses_and_their_messages(capsys, tmp_path):
    assert status_of() == 4
    assert capsys.readouterr().err.startswith("readtape_amd:")
    assert status_of("-tap", "-nrzi") == 4
    err = capsys.readouterr().err
    assert "*** No <basefilename> given" in err and "use: python -m readtape_amd" in err
    assert status_of("-tap", "a", "b") == 4
    assert "*** unknown parameter: a" in capsys.readouterr().err
    for h in ("-h", "-H", "-?"):
        assert status_of(h) == 1
        err = capsys.readouterr().err
        assert "use: python -m readtape_amd" in err and "csvtbin followed by readtape" in err and "peakstats.csv is not written" in err
    missing = str(tmp_path / "nothing")
    assert status_of("-nrzi", missing) == 99
    assert f'Unable to open input file "{missing}" .tbin or .csv' in capsys.readouterr().err
    bad = tmp_path / "bad.tbin"
    bad.write_bytes(b"NOTATBIN" + bytes(400))
    assert status_of("-nrzi", str(bad)) == 99
    assert ".tbin file missing TBINHDR tag" in capsys.readouterr().err


@pytest.mark.parametrize("arg", ["-showibg=5", "-SHOWIBG=0", "-sumt=s.txt", "-sumc=s.csv", "-adjskew", "-d", "-d3", "-D255"])
def test_options_that_are_parsed_but_not_built_end_the_run(arg, capsys):
    assert status_of("-nrzi", arg, "g") == 2
    err = capsys.readouterr().err
    assert err.startswith(arg + ": ") and err.count("\n") == 1


def test_out_of_range_values_of_unbuilt_options_are_bad_options():
    assert status_of("-showibg=-1", "g") == 99 and status_of("-d256", "g") == 99


# ---- parameter sets ----
PARMS = ("// a comment\n"
         "readtape -correct -linesize=80\n"
         "parms active, clk_window, clk_alpha, agc_window, agc_alpha, min_peak, clk_factor, pulse_adj, pkww_bitfrac, pkww_rise, midbit, z1pt, z2pt, id\n"
         "  readtape -EVEN\n"
         "{1, 0, 0.2, 0, 0.8, 0.5, 0, 0.3, 1.395, 0.3, 0.5, 1.45, 2.35, PRM}\n")


def test_readtape_lines_of_a_parms_text_are_options():
    assert cli.parms_options(PARMS) == ["-correct", "-linesize=80", "-EVEN"]
    o = parse("-nrzi")[0]
    for a in cli.parms_options(PARMS):
        assert cli.parse_option(o, a)
    assert o.correct and o.even_parity and o.linesize == 80
    with pytest.raises(cli.CliExit) as e:
        cli.parse_option(o, "-nonsense")
    assert e.value.status == 99


def test_the_three_places_of_a_parms_file(tmp_path, monkeypatch):
    data, cwd = tmp_path / "data", tmp_path / "cwd"
    data.mkdir(), cwd.mkdir()
    monkeypatch.chdir(cwd)
    base = str(data / "g")
    assert cli.find_parms(base, tbin.MODE_NRZI) is None
    (cwd / "NRZI.parms").write_text(PARMS)
    (cwd / "PE.parms").write_text(PARMS)
    assert cli.find_parms(base, tbin.MODE_NRZI) == str(cwd / "NRZI.parms")
    assert cli.find_parms(base, tbin.MODE_PE) == str(cwd / "PE.parms")
    assert cli.find_parms(base, tbin.MODE_GCR) is None
    (data / "NRZI.parms").write_text(PARMS)
    assert cli.find_parms(base, tbin.MODE_NRZI) == str(data / "NRZI.parms")
    (data / "g.parms").write_text(PARMS)
    assert cli.find_parms(base, tbin.MODE_NRZI) == base + ".parms"
    assert cli.find_parms(base, tbin.MODE_PE) == base + ".parms"
    (cwd / "Whirlwind.parms").write_text(PARMS)
    assert cli.find_parms(str(data / "other"), tbin.MODE_WW) == str(cwd / "Whirlwind.parms")
    assert cli.find_parms("g", tbin.MODE_GCR) is None                         # (a bare name has no directory of its own)


def test_extensions_are_cut_in_any_case():
    assert cli.split_ext("a/b.TBIN") == ("a/b", ".TBIN") and cli.split_ext("b.Csv") == ("b", ".Csv") and cli.split_ext("b.tap") == ("b", ".tap")
    assert cli.split_ext("b.bin") == ("b.bin", "") and cli.split_ext("a.b/c") == ("a.b/c", "")


def test_every_command_line_of_the_examples_parses():
    lines = ["-v -m -ntrks=9 -pe -bpi=1600 -ips=50 -order=01234576p -tap -ascii -linefeed -outp=results/ 1600bpi_ukn_6s.tbin",
             "-v -m -ntrks=9 -pe -bpi=1600 -ips=50 -tap -ebcdic -linesize=137 -outp=results/ LJS009_part1_39blks.tbin",
             "-whirlwind -v3 -fluxdir=auto -tap -deskew -octal2 -flexo -outp=results/ 132_pt1.tbin",
             "-v -m -nrzi -ips=50 -deskew -ebcdic -linefeed -outp=results/ PLAGO_beginning.tbin",
             "-v -m -nrzi -hex -ascii -outp=results/ Microdata_20blks.tbin",
             "-v -m -gcr -ips=50 -order=76543210p -zeros -correct -tap -ascii -linefeed -outp=results/ 1kblks_43blks.tbin",
             "-v -m -gcr -ips=50 -zeros -correct -tap -ascii -linefeed -outp=results/ sf93_8blks.tbin",
             "-v -gcr -ips=125 -differentiate -zeros -tap -ascii -outp=results/ analog.tbin",
             "-v -m -nrzi -ntrks=7 -order=543210p -tap -SDS -linesize=144 -outp=results/ SRI_SDS_102715028_4secs.tbin",
             "-v -m -nrzi -ntrks=7 -tap -outp=results/ tss_4secs.tbin"]
    for line in lines:
        o, rest = parse(*line.split())
        assert len(rest) == 1 and o.outp == "results/" and o.verbose
        assert cli.split_ext(rest[0])[1] == ".tbin"
        assert o.labels                                                        # (none of them says -nolabels)
