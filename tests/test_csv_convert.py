"""CSV -> TBIN on the host with the converter's window options, -graph and -redo (csvin.convert_csv / read_csv / convert_window; csrc/host/rt_csv.c):
the files are the reference converter's byte for byte (tests/golden/csvconv_*.npz, made by make_csvconv_golden.py), the closed-form window rule equals
the converter's two loops restated literally, what the option parser refuses is refused, and default options change nothing.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csv_shapes
import csvconv_util as U
from readtape_amd import csvin, tbin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_golden_files_byte_for_byte(name, tmp_path):
    z, kw = U.load(name)
    src, dst = str(tmp_path / "c.csv"), str(tmp_path / "c.tbin")
    open(src, "wb").write(z["csv"].tobytes())
    want = z["tbin"].tobytes()
    want_hdr, off = tbin.parse_header(want[:4096])
    hdr, info = csvin.convert_csv(src, dst, times=want_hdr.times, bpi=want_hdr.bpi, ips=want_hdr.ips, **kw)
    assert open(dst, "rb").read() == want
    assert open(str(tmp_path / "c.graph.csv"), "rb").read() == z["graph"].tobytes()
    # ... and the same through read_csv: the rows, and the graph as numbers
    hdr2, rows, info2 = csvin.read_csv(src, bpi=want_hdr.bpi, ips=want_hdr.ips, **kw)
    assert rows.tobytes() + b"\x00\x80" == want[off:] and info2["samples"] == rows.shape[0] == info["samples"]
    assert (hdr2.tstart_ns, hdr2.tdelta_ns, hdr2.flags) == (want_hdr.tstart_ns, want_hdr.tdelta_ns, want_hdr.flags)
    lines = z["graph"].tobytes().decode().splitlines()
    at, mx = info2["graph"]
    assert mx.dtype == np.float32 and [int(ln.split(",")[0]) for ln in lines] == list(at)
    assert [ln.split(", ")[1] for ln in lines] == ["%f" % v for v in mx]
    assert len(lines) == csvin.graph_lines(info["samples"], info["ended"], kw["graph"])
    assert not info["redone"]


def test_goldens_cover_what_they_are_meant_to():
    """The dropped line of a pass that ends on a full bin, K = 1 for a start time in front of the file, an empty graph."""
    z, kw = U.load("csvconv_start_end_graph100")
    n = (len(z["tbin"]) - tbin.parse_header(z["tbin"].tobytes()[:4096])[1] - 2) // 18
    assert n == 300 and z["graph"].tobytes().count(b"\n") == 2
    z, kw = U.load("csvconv_start_before_t0")
    assert (len(z["tbin"]) - tbin.parse_header(z["tbin"].tobytes()[:4096])[1] - 2) // 18 == U.CASES["csvconv_start_before_t0"][0] - 1
    assert len(U.load("csvconv_graph_bin_too_big")[0]["graph"]) == 0 and len(U.load("csvconv_stopaft1")[0]["graph"]) == 0


@pytest.fixture(scope="module")
def redo_csv(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("redo") / "r.csv")
    text = U.redo_text()
    assert U.sha(text) == str(U.load("csvconv_redo")[0]["csv_sha256"])
    open(path, "wb").write(text)
    return path


@pytest.mark.parametrize("name", ["csvconv_redo", "csvconv_redo_not"])
def test_redo_recipe(name, redo_csv, tmp_path):
    """A file that clips only behind the pre-read's million lines: with -redo the second pass has the larger full scale and the five skipped lines back."""
    z, kw = U.load(name)
    head = z["header"].tobytes()
    want_hdr, off = tbin.parse_header(head + bytes(64))
    dst = str(tmp_path / "r.tbin")
    hdr, info = csvin.convert_csv(redo_csv, dst, times=want_hdr.times, **kw)
    got = open(dst, "rb").read()
    assert got[: len(head)] == head
    assert (len(got) - len(head), U.sha(got[len(head):])) == (int(z["payload_bytes"]), str(z["payload_sha256"]))
    assert open(str(tmp_path / "r.graph.csv"), "rb").read() == z["graph"].tobytes()
    redo = name == "csvconv_redo"
    assert info["redone"] == redo and info["skipped"] == 5 and info["samples"] == U.REDO_LINES - (0 if redo else 5)
    assert (info["clipped_samples"] > 0) == (not redo) and info["clipped_samples"] == info["too_big"] + info["too_small"]


def test_window_rule_equals_the_two_loops():
    lib = csvin._lib()
    w = csvin._ConvWindow()
    T0, cases = 9_990_000, 0
    ns = lambda x: int(float(np.float32(x)) * 1e9)
    for sub in (1, 2, 3):
        D = 1000 * sub
        for nlines in range(0, 41):
            for skip in (0, 1, 2, 7, 39, 40, 41):
                for start in (0.0, 0.01, 0.010001, 0.01002, 0.0101):
                    for end in (0.0, 0.010001, 0.010005, 0.01002, 0.5):
                        for stopaft in (None, 1, 2, 5, 13, 40):
                            want = U.literal_window(T0, D, nlines, sub, skip, ns(start) if start else 0, ns(end) if end else None, stopaft)
                            rc = lib.rt_csv_convert_window(T0, D, nlines, sub, skip, start, end, stopaft or 0, w)
                            cases += 1
                            if want is None:
                                assert rc == -5, (sub, nlines, skip, start, end, stopaft, rc)
                                continue
                            assert rc == 0
                            got = (w.skipped, w.first_line if w.count else None, w.count, csvin.ENDED[w.ended])
                            assert got == want, (sub, nlines, skip, start, end, stopaft, got, want)
    assert cases > 100000
    # a clock that stands still never reaches a start time; a period of 0 with an end time in front of the file ends on the first sample
    assert lib.rt_csv_convert_window(1000, 0, 10, 1, 0, 0.01, 0.0, 0, w) == -5
    assert lib.rt_csv_convert_window(20_000_000, 0, 10, 1, 0, 0.0, 0.01, 0, w) == 0 and (w.count, w.ended) == (1, 2)
    assert U.literal_window(20_000_000, 0, 10, 1, 0, 0, ns(0.01), None) == (0, 0, 1, "endtime")
    d = csvin.convert_window(T0, 1000, 1500, skip=10, stopaft=300)
    assert d == dict(skipped=10, first_line=10, count=300, ended="stopaft")


def test_refusals(tmp_path):
    path = str(tmp_path / "c.csv")
    open(path, "wb").write(csv_shapes.shape("x", csv_shapes.plain_lines(30))["text"])
    for kw in (dict(skip=-1), dict(stopaft=0), dict(stopaft=-3), dict(starttime=0.009), dict(starttime=1000.5), dict(endtime=0.001), dict(endtime=2000.0),
               dict(starttime=0.5, endtime=0.5), dict(starttime=0.6, endtime=0.5), dict(graph=-1), dict(graph=1 << 31), dict(skip=31), dict(starttime=0.02),
               dict(ntrks=0), dict(ntrks=20)):
        with pytest.raises(ValueError):
            csvin.read_csv(path, **kw)
        with pytest.raises(ValueError):
            csvin.convert_csv(path, str(tmp_path / "o.tbin"), **kw)
    assert csvin.read_csv(path, skip=30)[1].shape == (0, 9)                          # the skip ends with the file: nothing left, and no error
    with pytest.raises(OSError):
        csvin.convert_csv(str(tmp_path / "none.csv"), str(tmp_path / "o.tbin"))
    with pytest.raises(OSError):
        csvin.convert_csv(path, str(tmp_path / "no_such_dir" / "o.tbin"))


@pytest.mark.parametrize("sh", [s for s in csv_shapes.all_shapes() if s["name"] in ("numbers", "clip_rails", "clip_rails_invert", "perm7_sub2_invert", "crlf")], ids=lambda s: s["name"])
def test_default_options_are_the_loader(sh, tmp_path):
    """read_csv without the new options returns rt_csv_load's rows and clip count (the loader as it was), and convert_csv writes exactly them."""
    import ctypes as C
    path = str(tmp_path / "c.csv")
    open(path, "wb").write(sh["text"])
    kw = sh["kw"]
    hdr, rows, info = csvin.read_csv(path, _preread_rows=sh["preread"], **kw)
    lib = csvin._lib()
    perm = csvin._order_flags(kw["ntrks"], tbin.MODE_NRZI, kw.get("order"), kw.get("invert", False))[0]
    old = np.empty((rows.shape[0] + 8, kw["ntrks"]), dtype=np.int16)
    clipped = C.c_int64()
    n = lib.rt_csv_load(path.encode(), kw["ntrks"], perm, int(kw.get("invert", False)), kw.get("scale", 1.0), kw.get("subsample", 1), hdr.maxvolts, old.ctypes.data,
                        old.shape[0], C.byref(clipped))
    assert n == rows.shape[0] and np.array_equal(old[:n], rows)
    assert info["clipped_samples"] == clipped.value == info["too_big"] + info["too_small"]
    assert (info["skipped"], info["samples"], info["redone"], info["ended"]) == (0, n, False, "file") and "graph" not in info
    dst = str(tmp_path / "c.tbin")
    hdr2, _ = csvin.convert_csv(path, dst, _preread_rows=sh["preread"], **kw)
    assert hdr2 == hdr and open(dst, "rb").read() == tbin.pack_header(hdr) + rows.tobytes() + b"\x00\x80"
    assert not os.path.exists(str(tmp_path / "c.graph.csv"))


def test_redo_on_a_short_text(tmp_path):
    """A 300-line text that clips at line 200 with a pre-read of 50 lines: both rails counted, the second pass by -starttime alone."""
    lines = csv_shapes.plain_lines(300, amp=2.0)
    lines[200] = csv_shapes.data_line(200, [9.0, -8.0, 0, 0, 0, 0, 0, 0, 7.5])
    path = str(tmp_path / "c.csv")
    open(path, "wb").write(csv_shapes.shape("x", lines)["text"])
    h1, r1, i1 = csvin.read_csv(path, _preread_rows=50, skip=7, graph=64)
    assert (i1["too_big"], i1["too_small"], i1["redone"], i1["samples"]) == (2, 1, False, 293)
    h2, r2, i2 = csvin.read_csv(path, _preread_rows=50, skip=7, graph=64, redo=True)
    assert i2["redone"] and i2["clipped_samples"] == 0 and (i2["skipped"], i2["samples"]) == (7, 300)
    assert np.float32(h2.maxvolts) == np.float32(9.1) and h2.maxvolts > h1.maxvolts
    assert np.array_equal(i1["graph"][0], i2["graph"][0]) and i1["graph"][1].tobytes() == i2["graph"][1].tobytes() and len(i1["graph"][0]) == 293 // 64
    h3, r3, i3 = csvin.read_csv(path, _preread_rows=50, skip=7, starttime=0.0125125, redo=True)           # K = 10 lines on either pass
    assert (i3["skipped"], i3["samples"], i3["redone"]) == (10, 290, True) and np.array_equal(r3, r2[10:])
