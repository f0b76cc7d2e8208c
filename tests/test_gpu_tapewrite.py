"""The tape writer on the GPU: the kernel (readtape_amd/csrc/rtfe_tapewrite.hip) against the host renderer byte for byte on tests/tapewrite_util.py's cases,
write_tbin_device against write_tbin, and the round trip - a tape rendered on the device and decoded from the same tensor gives back the image it was
written from."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tapewrite_util as U

from readtape_amd import frontend, ingest, pipeline, tapewrite as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return U.Device(frontend.TorchBackend())


@pytest.mark.parametrize("name", list(U.CASES))
def test_case(name, dev):
    U.CASES[name](dev)


def test_file_in_windows(dev, tmp_path):
    U.file_case(dev, tmp_path)


def _options(extra):
    return pipeline.DecodeOptions(multiple_tries=True, even_parity="-even" in extra)


@pytest.mark.parametrize("name", list(U.TAPES))
def test_round_trip_resident(name, dev, tmp_path):
    """render_device -> pipeline.decode_tape on the same tensor (no host copy of the rows), the command line's default options (-m): the image comes back"""
    spec_fn, items, extra = U.TAPES[name]
    plan = W.encode(items, spec_fn())
    rows = W.render_device(plan)
    assert rows.is_cuda
    tap = str(tmp_path / "t.tap")
    stats, _ = pipeline.decode_tape(plan.spec.header(), rows, tap, opts=_options(extra))
    assert U.same_items(W.tap_image(items), open(tap, "rb").read()) is None, U.same_items(W.tap_image(items), open(tap, "rb").read())
    assert stats["blocks_with_errors"] == 0 and stats["blocks_unusable"] == 0 and stats["all_ok"], stats


def test_round_trip_through_the_written_file(dev, tmp_path):
    """write_tbin_device, then ingest.decode_file_windows on the file"""
    spec_fn, items, extra = U.TAPES["nrzi9"]
    path, tap = str(tmp_path / "t.tbin"), str(tmp_path / "t.tap")
    W.write_tbin_device(items, path, spec_fn(), window_rows=50_000)
    stats = ingest.decode_file_windows(path, tap_path=tap, labels=False, opts=_options(extra), window_rows=1 << 15, halo_rows=1 << 17)      # (four windows; the halo is longer than the longest block)
    assert stats["windows"] >= 3
    assert U.same_items(W.tap_image(items), open(tap, "rb").read()) is None
    assert stats["blocks_with_errors"] == 0 and stats["all_ok"], stats
