"""The device CSV export (csvout.write_csv_device; kernels in readtape_amd/csrc/rtfe_csvout.hip) with the kernels run by the CPU emulator: the goldens are the
reference converter's text, and every other case - every int16 code, every track count, the seams where a field grows, the ties of the time field, a text
that does not fit - is the host writer's text, byte for byte.  The cases are tests/csvout_util.py's, shared with tests/test_gpu_csvout.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csvout_util as U
from emul_util import NumpyBackend, build_emul


@pytest.mark.parametrize("name", U.EXPECTED_GOLDENS)
def test_golden_is_the_reference_text(name, tmp_path):
    U.run_golden(name, tmp_path, NumpyBackend(), build_emul())


@pytest.mark.parametrize("mv,inv", U.EVERY_CODE)
def test_every_code(mv, inv, tmp_path):
    U.run_every_code(mv, inv, tmp_path, NumpyBackend(), build_emul())


@pytest.mark.parametrize("ntrks", range(1, 20))
def test_every_track_count(ntrks, tmp_path):
    U.run_ntrks(ntrks, tmp_path, NumpyBackend(), build_emul())


def test_voltage_width_seams(tmp_path):
    U.run_voltage_width_seams(tmp_path, NumpyBackend(), build_emul())


def test_time_width_seams_and_the_path_taken(tmp_path):
    U.run_time_width_seams(tmp_path, NumpyBackend(), build_emul())


def test_time_ties_and_the_last_time(tmp_path):
    U.run_time_ties(tmp_path, NumpyBackend(), build_emul())


def test_a_text_that_does_not_fit(tmp_path):
    U.run_bounds(tmp_path, U.Format(NumpyBackend(), build_emul()))


def test_refusals():
    U.run_refusals(U.Format(NumpyBackend(), build_emul()))


@pytest.mark.parametrize("name", U.ROUNDTRIP)
def test_round_trip_through_the_device_ingest(name, tmp_path):
    U.run_round_trip(name, tmp_path, NumpyBackend(), build_emul())
