"""rtfe_csv_graph (readtape_amd/csrc/rtfe_csv.hip) and the device conversion with window options, -graph and -redo (csvin.read_csv_device /
convert_csv_device), the kernels run by the CPU emulator: the graph kernel alone against a numpy restatement in the same float32 operations, then the
device functions against the host's - rows, header, info, graph arrays, both files' bytes.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csv_shapes
import csvconv_util as U
from emul_util import NumpyBackend, build_emul
from readtape_amd import csvin

GRAPH_CASES = U.graph_cases()
SHAPES = [s for s in csv_shapes.all_shapes() if s["path"] == "device" and s["name"] in ("numbers", "clip_rails_invert", "perm7_sub2_invert", "crlf")]


@pytest.fixture(scope="module")
def graph():
    return U.Graph(NumpyBackend(), build_emul())


@pytest.mark.parametrize("case", GRAPH_CASES, ids=[c[0] for c in GRAPH_CASES])
def test_graph_kernel_alone(graph, case):
    U.run_graph_case(graph, case)


def test_graph_kernel_without_a_peak(graph):
    U.run_graph_case(graph, GRAPH_CASES[2], with_peak=False)
    U.run_graph_case(graph, GRAPH_CASES[0], with_peak=False)


def test_graph_refusals(graph):
    U.run_graph_refusals(graph)


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_golden_on_the_device_equals_the_host(name, tmp_path):
    z, kw = U.load(name)
    U.check_device_equals_host(name, z["csv"].tobytes(), kw, tmp_path, NumpyBackend(), build_emul())


@pytest.mark.parametrize("sh", SHAPES, ids=[s["name"] for s in SHAPES])
def test_shapes_with_window_options(sh, tmp_path):
    for opts in U.device_option_sets():
        U.check_device_equals_host(f"{sh['name']} {opts}", sh["text"], dict(sh["kw"], **opts), tmp_path, NumpyBackend(), build_emul(), windows=(4096, 1 << 28, 450),
                                   preread=sh["preread"])


def test_redo_on_the_device(tmp_path):
    """A 300-line text that clips at line 200, the pre-read 50 lines long: the second pass runs with the larger full scale and without the skip."""
    lines = csv_shapes.plain_lines(300, amp=2.0)
    lines[200] = csv_shapes.data_line(200, [9.0, -8.0, 0, 0, 0, 0, 0, 0, 7.5])
    text = csv_shapes.shape("x", lines)["text"]
    for opts in (dict(skip=7, graph=64, redo=True), dict(skip=7, graph=64), dict(skip=7, starttime=0.0125125, stopaft=250, graph=3, redo=True)):
        want = U.check_device_equals_host(f"redo {opts}", text, dict(ntrks=9, **opts), tmp_path, NumpyBackend(), build_emul(), preread=50)
        assert want[2]["redone"] == bool(opts.get("redo"))


def test_a_file_for_the_host_goes_to_the_host(tmp_path):
    """A line longer than fgets returns whole: read_csv's and convert_csv's results, path = "host"."""
    sh = next(s for s in csv_shapes.all_shapes() if s["path"] == "host")
    U.check_device_equals_host(sh["name"], sh["text"], dict(sh["kw"], skip=2, graph=3), tmp_path, NumpyBackend(), build_emul(), windows=(1 << 20,), preread=sh["preread"], path="host")
