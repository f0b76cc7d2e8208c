"""The device CSV export (csvout.write_csv_device; kernels in readtape_amd/csrc/rtfe_csvout.hip) on the GPU: the cases of tests/test_emul_csvout.py
(tests/csvout_util.py) - the goldens against the reference converter's text, everything else against the host writer - and a device tensor of several
pipelined windows.  Byte for byte; no tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csvout_util as U
from readtape_amd import frontend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return frontend.TorchBackend()


@pytest.mark.parametrize("name", U.EXPECTED_GOLDENS)
def test_golden_is_the_reference_text(name, tmp_path, be):
    U.run_golden(name, tmp_path, be)


@pytest.mark.parametrize("mv,inv", U.EVERY_CODE)
def test_every_code(mv, inv, tmp_path, be):
    U.run_every_code(mv, inv, tmp_path, be)


@pytest.mark.parametrize("ntrks", range(1, 20))
def test_every_track_count(ntrks, tmp_path, be):
    U.run_ntrks(ntrks, tmp_path, be)


def test_voltage_width_seams(tmp_path, be):
    U.run_voltage_width_seams(tmp_path, be)


def test_time_width_seams_and_the_path_taken(tmp_path, be):
    U.run_time_width_seams(tmp_path, be)


def test_time_ties_and_the_last_time(tmp_path, be):
    U.run_time_ties(tmp_path, be)


def test_a_text_that_does_not_fit(tmp_path, be):
    U.run_bounds(tmp_path, U.Format(be))


def test_refusals(be):
    U.run_refusals(U.Format(be))


@pytest.mark.parametrize("name", U.ROUNDTRIP)
def test_round_trip_through_the_device_ingest(name, tmp_path, be):
    U.run_round_trip(name, tmp_path, be)


def test_a_device_tensor_in_pipelined_windows(tmp_path, be):
    """2e5 rows that are already on the device, seven windows through the copy stream and the writer thread; the time crosses 1000 s in the fourth."""
    import torch
    rng = np.random.RandomState(21)
    rows = rng.randint(-32767, 32768, (200_003, 9)).astype(np.int16)
    hdr = U.hdr_for(tdelta=1285, tstart=10 ** 12 - 1285 * 100_000, maxvolts=5.0)
    d_rows = torch.from_numpy(rows).to(be.device)
    want, _ = U.host_text(tmp_path, hdr, rows, stagger=0.5, skip=11)
    got, info = U.device_text(tmp_path, be, None, hdr, d_rows, stagger=0.5, skip=11, window_rows=30_000)
    U.same(got, want, "pipelined")
    assert info["windows"] == 7 and info["path"] == "mixed" and info["ms"]["format"] > 0
