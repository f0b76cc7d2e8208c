"""The device text dump (textfile.write_text_device; kernels in readtape_amd/csrc/rtfe_textfile.hip) with the kernels run by the CPU emulator: the goldens are
the reference's text, and every other case - the record lengths around a line's end and around the prefix's widths, every number type alone and with a
character type, octal2 at odd sizes, the -dataspace cases, linefeeds at every place that matters, lines across the kernel's own cuts, a text that does not
fit - is the host writer's text, byte for byte.  The cases are tests/textfile_util.py's, shared with tests/test_gpu_textfile.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import textfile_util as U
from emul_util import NumpyBackend, build_emul


@pytest.mark.parametrize("name", U.EXPECTED_GOLDENS)
def test_golden_is_the_reference_text(name, tmp_path):
    U.run_golden(name, tmp_path, NumpyBackend(), build_emul())


@pytest.mark.parametrize("shape", U.OPTION_SHAPES, ids=repr)
def test_record_lengths_under_every_option_shape(shape, tmp_path):
    U.run_option_shape(shape, tmp_path, NumpyBackend(), build_emul())


def test_the_prefix_widens_and_the_longest_record(tmp_path):
    U.run_wide_prefix(tmp_path, NumpyBackend(), build_emul())


@pytest.mark.parametrize("shape", U.LINEFEED_SHAPES, ids=repr)
def test_linefeeds(shape, tmp_path):
    U.run_linefeed_shape(shape, tmp_path, NumpyBackend(), build_emul())


def test_lines_across_the_kernels_cuts(tmp_path):
    U.run_kernel_cuts(tmp_path, NumpyBackend(), build_emul())


def test_empty_images_and_a_missing_end(tmp_path):
    U.run_empty_and_missing_end(tmp_path, NumpyBackend(), build_emul())


def test_a_text_that_does_not_fit(tmp_path):
    U.run_bounds(tmp_path, U.Format(NumpyBackend(), build_emul()))


def test_refusals():
    U.run_refusals(U.Format(NumpyBackend(), build_emul()))
