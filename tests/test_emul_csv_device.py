"""The device CSV path (csvin.read_csv_device; kernels in readtape_amd/csrc/rtfe_csv.hip) with the kernels run by the CPU emulator: it makes of a
logic-analyser export the converter's .tbin (the goldens) and, shape for shape of tests/csv_shapes.py, exactly what the host loader read_csv makes -
header, every code, the clip count - whatever the window size.  No tolerance anywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csv_device_util as U
import csv_shapes
from emul_util import NumpyBackend, build_emul, emul_frontend
from readtape_amd import csvin, frontend

SHAPES = csv_shapes.all_shapes()


def test_the_shapes_mirror_the_kernels_constants():
    csv_shapes.check_constants()
    names = [s["name"] for s in SHAPES]
    assert len(set(names)) == len(names)
    assert all(len(s["windows"]) >= 2 for s in SHAPES if s["path"] == "device" and "branches" not in s)


@pytest.mark.parametrize("name", U.CSV_CASES)
def test_golden_csv_becomes_the_converters_tbin(name, tmp_path):
    U.check_golden_tbin(name, tmp_path, NumpyBackend(), build_emul())
    U.check_golden_tbin(name, tmp_path, NumpyBackend(), build_emul(), window_bytes=3001)


@pytest.mark.parametrize("sh", SHAPES, ids=[s["name"] for s in SHAPES])
def test_shape_equals_the_host_loader(sh, tmp_path):
    U.check_shape(sh, tmp_path, NumpyBackend(), build_emul())


def test_index_alone():
    U.run_index_cases(U.Index(NumpyBackend(), build_emul()))


def test_index_refuses_to_write_behind_starts_cap():
    U.run_starts_cap_cases(U.Index(NumpyBackend(), build_emul()))


def test_a_window_with_more_lines_than_guessed_is_indexed_again(tmp_path):
    """read_csv_device guesses a line per 8 bytes for the table of starts: a file of blank lines has more."""
    sh = csv_shapes.shape("blank_lines", [b"0.001, 1.5\n"] + [b"\n"] * 400 + [b"0.002, 2.5\n"], ntrks=1, windows=(1 << 20, 256))
    U.check_shape(sh, tmp_path, NumpyBackend(), build_emul())


def test_refusals():
    be, lib = NumpyBackend(), frontend._load_library(build_emul())
    dev = csvin._Dev(be, False)
    text, starts, out = dev.alloc(64), dev.alloc(64), dev.alloc(64)
    p = be.ptr
    perm = (C.c_int * 3)(0, 3, 1)
    assert lib.rtfe_csv_parse(p(text), p(starts), 0, 1, 1, 0, None, 0, 1.0, 1.0, p(out), p(out), None) == -3 and b"ntrks" in lib.rtfe_last_error()
    assert lib.rtfe_csv_parse(p(text), p(starts), 0, 1, 1, 20, None, 0, 1.0, 1.0, p(out), p(out), None) == -3
    assert lib.rtfe_csv_parse(p(text), p(starts), 0, 1, 1, 3, perm, 0, 1.0, 1.0, p(out), p(out), None) == -4 and b"perm[1]" in lib.rtfe_last_error()
    assert lib.rtfe_csv_peak(p(text), p(starts), 0, 1, 20, 1.0, p(out), None) == -3
    assert lib.rtfe_csv_index(p(text) + 4, 8, 1, p(starts), 4, p(out), 64, p(out), None) == -31
    assert lib.rtfe_csv_index(p(text), 1 << 32, 1, p(starts), 4, p(out), 64, p(out), None) == -35
    assert lib.rtfe_abi_version() == 6 and lib.rtfe_kernel_count() == 12


def test_refusals_of_read_csv_device(tmp_path):
    path = str(tmp_path / "c.csv")
    open(path, "wb").write(csv_shapes.shape("x", csv_shapes.plain_lines(5))["text"])
    for kw in (dict(ntrks=0), dict(ntrks=20)):
        with pytest.raises(ValueError):
            csvin.read_csv_device(path, _lib_path=build_emul(), _backend=NumpyBackend(), **kw)
    with pytest.raises(OSError):
        csvin.read_csv_device(str(tmp_path / "none.csv"), _lib_path=build_emul(), _backend=NumpyBackend())


def test_golden_through_the_emulated_front_end_to_its_tap(tmp_path):
    U.check_golden_tap("csv_nrzi7_order_late", tmp_path, NumpyBackend(), build_emul(), fe_factory=emul_frontend)
