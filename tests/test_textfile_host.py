"""The interpreted text dump on the host (textfile.write_text / read_tap; csrc/host/rt_textfile.c, rt_tapread.c, and the decode path's text file): the
file is the reference's -tapread / -textfile output, byte for byte - against the goldens tests/make_textfile_golden.py made with the reference itself, the
images it stops on included.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import textfile_util as U
from readtape_amd import textfile
from readtape_amd.textfile import TextOptions


def test_the_goldens_are_all_there():
    assert set(U.EXPECTED_GOLDENS) | set(U.DECODE_GOLDENS) <= set(U.GOLDENS)


@pytest.mark.parametrize("name", U.TAP_GOLDENS)
def test_golden_is_the_reference_text(name, tmp_path):
    g = U.load_golden(name)
    assert g["status"] == 0
    opts, ntrks = U.opts_from_args(g["opts"])
    got, fname, err = U.host_text(tmp_path, g["tap"], opts, ntrks)
    assert err is None and fname == g["name"]
    U.same(got, g["txt"], name)


@pytest.mark.parametrize("name", U.FATAL_GOLDENS)
def test_what_the_reference_stops_on(name, tmp_path):
    """The reader's fatal cases: the error is raised, and the file holds what the reference had written when it exited."""
    g = U.load_golden(name)
    assert g["status"] != 0
    opts, ntrks = U.opts_from_args(g["opts"])
    got, fname, err = U.host_text(tmp_path, g["tap"], opts, ntrks)
    assert isinstance(err, textfile.TapFormatError) and fname == g["name"]
    U.same(got, g["txt"], name)
    with pytest.raises(textfile.TapFormatError) as e:
        textfile.read_tap(g["tap"])
    want = {"fatal_pad5": 5, "fatal_gap": 2, "fatal_class": 2, "fatal_zero": 3, "fatal_big": 4, "fatal_short": 1, "fatal_no_trailer": 1, "fatal_sizes": 3}[name]
    assert e.value.status == want == err.status, (e.value.status, str(e.value))


def test_the_item_table():
    img = U.MARK + U.rec(b"abc", err=True) + U.rec(b"defg", pad=3) + U.MARK + U.rec(b"z")
    it = textfile.read_tap(img)
    assert [(int(i["kind"]), int(i["offset"]), int(i["length"]), int(i["flag"])) for i in it] == [
        (textfile.MARK, 0, 0, 0), (textfile.RECORD, 8, 3, 1), (textfile.RECORD, 20, 4, 0), (textfile.MARK, 31, 0, 0), (textfile.RECORD, 39, 1, 0),
        (textfile.MESSAGE, len(img), 0, 0)]
    assert len(textfile.read_tap(U.EOM)) == 0 and len(textfile.read_tap(b"")) == 1
    assert textfile.ITEM.itemsize == 16


def test_names_and_defaults(tmp_path):
    assert textfile.text_name("b", TextOptions("hex", "ebcdic")) == "b.hex.EBCDIC.txt"
    assert textfile.text_name("b", TextOptions("octal2", "flexo")) == "b.octal2.flexo.txt"
    assert textfile.text_name("b", TextOptions(None, "sds")) == "b.SDS.txt"
    assert textfile.text_name("b", TextOptions("octal")) == "b.octal.txt"
    assert textfile.text_name("b", TextOptions()) == "b.txt"
    for bad in (TextOptions("hex", linesize=3), TextOptions("hex", linesize=401), TextOptions("hex", dataspace=401), TextOptions("decimal"), TextOptions(char="latin1")):
        with pytest.raises(ValueError):
            textfile.write_text(U.EOM, str(tmp_path / "g"), bad)
    with pytest.raises(OSError):
        textfile.write_text(U.EOM, str(tmp_path / "none" / "g"), TextOptions("hex"))
    # octal2 spaces its words apart unless told otherwise; the title says which options were in force
    for opts, line in ((TextOptions("octal2"), b"using text options -octal2   -linesize=64 -dataspace=2\n"), (TextOptions("octal2", dataspace=0), b"using text options -octal2   -linesize=64\n"),
                       (TextOptions("hex", "ascii", linefeed=True), b"using text options -hex -ASCII -newline -linesize=32\n")):
        got, _, _ = U.host_text(tmp_path, U.EOM, opts)
        assert got.split(b"\n", 1)[1].startswith(line), got


def _tape(tkey):
    from readtape_amd import tbin
    t = np.load(os.path.join(U.GOLDEN, f"tape_{tkey}.npz"))
    ntrks, tdelta, mode, tstart = (int(x) for x in t["hdr"][:4])
    flags = int(t["hdr"][4]) if t["hdr"].size > 4 else 0
    maxvolts, bpi, ips = (float(x) for x in t["hdrf"])
    trkorder = str(t["trkorder"]) if "trkorder" in t.files else ""
    return tbin.TbinHeader(ntrks=ntrks, tdelta_ns=tdelta, maxvolts=maxvolts, mode=mode, bpi=bpi, ips=ips, tstart_ns=tstart, flags=flags, trkorder=trkorder), t["rows"]


@pytest.mark.parametrize("name", sorted(U.DECODE_GOLDENS))
def test_the_decode_path_writes_the_reference_text(name, tmp_path):
    """decode_tape(..., textfile=) on the emulated front end: the verbose layout beside the .tap, both the reference's; -addparity on a 7-track tape."""
    from emul_util import emul_frontend
    from readtape_amd import pipeline
    g = U.load_golden(name)
    hdr, rows = _tape(g["tape"])
    opts, _ = U.opts_from_args(g["opts"])
    base = str(tmp_path / "g")
    dopts = pipeline.DecodeOptions(add_parity="-addparity" in g["ref_opts"])
    pipeline.decode_tape(hdr, rows, base + ".tap", log_path=base + ".log", opts=dopts, fe_factory=emul_frontend, textfile=opts, created=U.DATE)
    assert open(base + ".tap", "rb").read() == g["tapout"]
    name_ = textfile.text_name(base, opts)
    assert os.path.basename(name_)[2:] == g["name"]
    body, date = U.cut_date(open(name_, "rb").read())
    assert date == b"created by readtape version 3.18 on " + U.DATE.encode()
    U.same(body.replace(base.encode(), b"g"), g["txt"], name)
    assert f'creating file "{name_}"' in open(base + ".log").read()
    if dopts.add_parity:                                  # the parity bit is in the .tap's bytes (and not in the text's)
        plain = str(tmp_path / "p")
        pipeline.decode_tape(hdr, rows, plain + ".tap", fe_factory=emul_frontend)
        a, b = textfile.read_tap(base + ".tap"), textfile.read_tap(plain + ".tap")
        assert [tuple(x) for x in a] == [tuple(x) for x in b]
        da, db = np.fromfile(base + ".tap", np.uint8), np.fromfile(plain + ".tap", np.uint8)
        rec0 = a[a["kind"] == textfile.RECORD][0]
        sl = slice(int(rec0["offset"]), int(rec0["offset"]) + int(rec0["length"]))
        assert np.array_equal(da[sl] & 0x3f, db[sl]) and (da[sl] & 0x40).any() and not (db[sl] & 0x40).any()


def test_addparity_is_refused_for_nine_tracks(tmp_path):
    from readtape_amd import pipeline
    hdr, rows = _tape("case_nrzi9")
    with pytest.raises(ValueError, match="addparity"):
        pipeline.decode_tape(hdr, rows, str(tmp_path / "g.tap"), opts=pipeline.DecodeOptions(add_parity=True))
