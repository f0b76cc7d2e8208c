"""Whirlwind with -zeros and / or -differentiate on the MI355X (run with -m gpu): the cases of tests/test_emul_ww_detectors.py through the
real k_ww_det (fe_factory=None) - the reference's .tap bytes, block lines and every field of its event dump, both chunk sizes, the
far-zero tape included - and the new entry points from a plain-C caller."""
import os
import subprocess

import pytest

from test_emul_ww_detectors import WW_DETECTOR_CASES, check_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_rows", [4096, 300])
@pytest.mark.parametrize("name", WW_DETECTOR_CASES)
def test_whirlwind_detectors_match_the_reference_on_the_gpu(name, chunk_rows, tmp_path, gpu):
    check_case(name, chunk_rows, tmp_path, None)


def build_ww_client(out_dir):
    """gcc (C, not C++) on tests/abi_ww_client.c: the header's Whirlwind detector section as a C translation unit, linked against librtfe.so."""
    from readtape_amd import build
    build.build_frontend()
    exe = os.path.join(str(out_dir), "abi_ww_client")
    subprocess.run(["gcc", "-std=gnu99", "-Wall", "-Werror=implicit-function-declaration", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT}/include", "-I/opt/rocm/include",
                    "-o", exe, os.path.join(ROOT, "tests", "abi_ww_client.c"), f"-L{ROOT}/readtape_amd", "-lrtfe", "-L/opt/rocm/lib", "-lamdhip64",
                    f"-Wl,-rpath,{ROOT}/readtape_amd", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_the_detector_entry_points_compile_as_c_and_link(tmp_path):
    assert os.path.exists(build_ww_client(tmp_path))


@pytest.mark.gpu
def test_a_c_client_scans_with_the_detector_entry_points(tmp_path, gpu):
    p = subprocess.run([build_ww_client(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr + p.stdout
    tag, kind, nbytes, nev = p.stdout.split()
    assert (tag, int(kind), int(nbytes)) == ("ok", 2, 432) and int(nev) > 20          # a square wave of 51 edges on track 1
