"""The device text dump (textfile.write_text_device; kernels in readtape_amd/csrc/rtfe_textfile.hip) on the GPU: the cases of tests/test_emul_textfile.py
(tests/textfile_util.py) - the goldens against the reference's text, everything else against the host writer - and an image of 2e5 records through several
pipelined windows.  Byte for byte; no tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import textfile_util as U
from readtape_amd import frontend
from readtape_amd.textfile import TextOptions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return frontend.TorchBackend()


@pytest.mark.parametrize("name", U.EXPECTED_GOLDENS)
def test_golden_is_the_reference_text(name, tmp_path, be):
    U.run_golden(name, tmp_path, be)


@pytest.mark.parametrize("shape", U.OPTION_SHAPES, ids=repr)
def test_record_lengths_under_every_option_shape(shape, tmp_path, be):
    U.run_option_shape(shape, tmp_path, be)


def test_the_prefix_widens_and_the_longest_record(tmp_path, be):
    U.run_wide_prefix(tmp_path, be)


@pytest.mark.parametrize("shape", U.LINEFEED_SHAPES, ids=repr)
def test_linefeeds(shape, tmp_path, be):
    U.run_linefeed_shape(shape, tmp_path, be)


def test_lines_across_the_kernels_cuts(tmp_path, be):
    U.run_kernel_cuts(tmp_path, be)


def test_empty_images_and_a_missing_end(tmp_path, be):
    U.run_empty_and_missing_end(tmp_path, be)


def test_a_text_that_does_not_fit(tmp_path, be):
    U.run_bounds(tmp_path, U.Format(be))


def test_refusals(be):
    U.run_refusals(U.Format(be))


def test_an_image_of_2e5_records_in_pipelined_windows(tmp_path, be):
    """2e5 records of 1 .. 120 bytes (12 MB of data, 45 MB of text), marks and flagged records among them, seven windows through the copy stream and the
    writer thread; then the same image with -linefeed, where the stretch table is made on the device."""
    rng = np.random.RandomState(33)
    lens = rng.randint(1, 121, 200_000)
    data = rng.randint(0, 256, int(lens.sum())).astype(np.uint8).tobytes()
    parts, at = [], 0
    for k, n in enumerate(lens):
        parts.append(U.rec(data[at: at + n], err=k % 97 == 0))
        if k % 1000 == 999:
            parts.append(U.MARK)
        at += n
    img = b"".join(parts) + U.EOM
    info = U.run_same_as_host(tmp_path, be, None, img, TextOptions("hex", "ebcdic"), what="pipelined", window_bytes=2 << 20)
    assert info["windows"] == 8 and info["items"] == 200_200 and info["bytes"] > 40e6 and info["ms"]["format"] > 0 and info["ms"]["copy"] > 0, info
    info = U.run_same_as_host(tmp_path, be, None, img, TextOptions("octal2", "flexo", 16, linefeed=True), what="pipelined, -linefeed", window_bytes=4 << 20)
    assert info["windows"] == 4, info
