"""The CSV export on the host (csvout.write_csv / export_window; csrc/host/rt_csvout.c): the text is the reference converter's -read, byte for byte - against
the goldens tests/make_csvout_golden.py made with the reference itself, and against the Python model of that text on random tapes.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csvout_util as U
from readtape_amd import csvin, csvout, tbin


def test_the_goldens_are_all_there():
    assert U.GOLDENS == U.EXPECTED_GOLDENS


@pytest.mark.parametrize("name", U.EXPECTED_GOLDENS)
def test_write_csv_is_the_reference_text(name, tmp_path):
    hdr, rows, kw, want = U.load_golden(name)
    assert rows.shape[0] <= 300
    got, info = U.host_text(tmp_path, hdr, rows, **kw)
    U.same(got, want, name)
    assert info["rows"] == want.count(b"\n") - 2
    U.same(U.model_text(hdr, rows, **kw), want, name + " (model)")


@pytest.mark.parametrize("name", [n for n in U.EXPECTED_GOLDENS if n.startswith("win_")])
def test_export_window_is_the_reference_window(name):
    """first and count from the reference's own timestamps: the first printed time names the first row, the line count the number of rows."""
    hdr, rows, kw, want = U.load_golden(name)
    lines = want.split(b"\n")[2:-1]
    first, count = csvout.export_window(hdr, rows.shape[0], **{k: v for k, v in kw.items() if k in ("skip", "starttime", "endtime", "stopaft")})
    assert count == len(lines) and 0 < count < rows.shape[0]
    assert lines[0].startswith(b"%12.8f, " % ((hdr.tstart_ns + first * hdr.tdelta_ns) / 1e9))


def test_export_window_rules():
    hdr = U.hdr_for(tdelta=100_000, tstart=1_000_000)
    W = lambda n, **kw: csvout.export_window(hdr, n, **kw)
    assert W(300) == (0, 300) and W(0) == (0, 0)
    assert W(300, skip=1) == (1, 299) and W(300, skip=300) == (300, 0) and W(300, skip=1000) == (300, 0)
    assert W(300, starttime=0.0005) == (1, 299)                      # a do-while: one row goes although the first is late enough
    assert W(300, starttime=0.011) == (100, 200)                     # (float)0.011 -> 10999999 ns: row 100 is at 11000000
    assert W(300, stopaft=1) == (0, 1) and W(300, stopaft=300) == (0, 300) and W(300, stopaft=301) == (0, 300)
    assert W(300, endtime=0.0005) == (0, 1)                          # the row that crosses endtime is still printed
    assert W(300, endtime=0.011) == (0, 100)                         # rows 0 .. 99: behind row 99 the clock reads 11000000 > 10999999
    assert W(300, skip=150, starttime=0.011, endtime=0.012, stopaft=7) == (150, 1)
    with pytest.raises(ValueError):
        W(-1)


@pytest.mark.parametrize("seed", range(6))
def test_write_csv_is_the_model_on_random_tapes(seed, tmp_path):
    rng = np.random.RandomState(100 + seed)
    ntrks = int(rng.randint(1, 20))
    rows = rng.randint(-32768, 32768, (int(rng.randint(1, 400)), ntrks)).astype(np.int16)
    rows[rows[:, 0] == -32768, 0] = 5
    rows[rng.randint(0, rows.shape[0])] = rng.randint(-2, 3, ntrks)
    hdr = U.hdr_for(ntrks=ntrks, tdelta=int(rng.choice([1, 1285, 1000, 3906250, 4_000_000_000])), maxvolts=float(rng.choice([0.1, 1.0, 3.3, 15.0, 250.0])),
                    invert=bool(seed & 1), tstart=int(rng.choice([0, 5, 1953125, 999_999_999_990, 10 ** 13 - 3, 10 ** 15])))
    order = None
    if 2 <= ntrks <= 11 and seed % 3 == 0:
        p = rng.permutation(ntrks)
        order = "".join("p" if t == ntrks - 1 else str(t) for t in p)
    kw = dict(order=order, stagger=float(rng.choice([0.0, 0.140625, 33.3, -7.77])))
    if seed % 2:
        kw.update(skip=int(rng.randint(0, 5)), stopaft=int(rng.randint(1, 500)))
    got, _ = U.host_text(tmp_path, hdr, rows, **kw)
    U.same(got, U.model_text(hdr, rows, **kw), seed)


def test_write_csv_refusals(tmp_path):
    rows = np.zeros((4, 9), np.int16)
    with pytest.raises(ValueError):
        csvout.write_csv(str(tmp_path / "a.csv"), U.hdr_for(), rows, order="01234")
    with pytest.raises(OSError):
        csvout.write_csv(str(tmp_path / "none" / "a.csv"), U.hdr_for(), rows)


@pytest.mark.parametrize("name", U.ROUNDTRIP)
def test_the_reference_text_reads_back_to_the_rows(name, tmp_path):
    """What makes a golden a round-trip case: read_csv on the reference's own text, at the header's full scale, gives the tape's rows."""
    hdr, rows, kw, want = U.load_golden(name)
    path = str(tmp_path / "ref.csv")
    open(path, "wb").write(want)
    hdr2, rows2, _ = csvin.read_csv(path, ntrks=hdr.ntrks, mode=hdr.mode, maxvolts=hdr.maxvolts, invert=bool(hdr.flags & tbin.FLAG_INVERTED), **kw)
    assert np.float32(hdr2.maxvolts) == np.float32(hdr.maxvolts) and np.array_equal(rows2, rows)
