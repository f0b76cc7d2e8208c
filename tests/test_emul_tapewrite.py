"""The device tape renderer (tapewrite.render_device, write_tbin_device; the kernel in readtape_amd/csrc/rtfe_tapewrite.hip) run by the CPU emulator and held
against the host renderer byte for byte on tests/tapewrite_util.py's cases, shared with tests/test_gpu_tapewrite.py; and the command line's --write."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tapewrite_util as U
from emul_util import NumpyBackend, build_emul

from readtape_amd import cli, tapewrite as W


def device():
    return U.Device(NumpyBackend(), build_emul())


@pytest.mark.parametrize("name", list(U.CASES))
def test_case(name):
    U.CASES[name](device())


def test_file_in_windows(tmp_path):
    U.file_case(device(), tmp_path)


def test_span_rows():
    d = device()
    assert all(d.span(n) > 0 and d.span(n) % 8 == 0 for n in range(1, 20)) and d.span(0) == 0 and d.span(20) == 0


def _cli(args, **kw):
    out = io.StringIO()
    return cli.main(args, out=out, **kw), out.getvalue()


def test_cli_write(tmp_path, monkeypatch):
    """--write=host and, with the emulator's library, --write: the file is write_tbin's"""
    base = str(tmp_path / "t")
    items = [("mark",), ("block", U.payload(1, 50)), ("block", U.payload(2, 7))]
    open(base + ".tap", "wb").write(W.tap_image(items))
    dev = (build_emul(), NumpyBackend())
    for args, spec in ((["-nrzi"], W.nrzi_spec()), (["-pe", "--seed=4", "--noise=5", "--jitter=0.01"], W.pe_spec(seed=4, noise_mv=5.0, jitter=float(np.float32("0.01")))),
                       (["-gcr", "--gap=2000", "--tdelta=200"], W.gcr_spec(gap_samples=2000, tdelta_ns=200)), (["-nrzi", "-bpi=556", "-ips=75"], W.nrzi_spec(bpi=556.0, ips=75.0)),
                       (["-nrzi", "-ntrks=9", "-even"], W.nrzi_spec(even=True))):
        W.write_tbin(base + ".tap", base + ".want.tbin", spec)
        want = open(base + ".want.tbin", "rb").read()
        for how, tag, name in (("--write=host", "host", base), ("--write", "dev", base + ".tap")):
            status, console = _cli([how] + args + [f"-outf={base}.{tag}", name], device=dev)
            assert status == 0 and "created" in console, console
            assert open(f"{base}.{tag}.tbin", "rb").read() == want, (how, args)
    monkeypatch.chdir(tmp_path)                                                # -outp= goes in front of the base name; -q says nothing
    W.write_tbin(base + ".tap", base + ".want.tbin", W.nrzi_spec())
    status, console = _cli(["--write=host", "-q", "-nrzi", "-outp=x_", "t"], device=dev)
    assert status == 0 and console == "" and open("x_t.tbin", "rb").read() == open(base + ".want.tbin", "rb").read()


@pytest.mark.parametrize("args,word", [(["-whirlwind"], "Whirlwind"), ([], "-nrzi, -pe or -gcr"), (["-pe", "-even"], "even parity"), (["-nrzi", "-ntrks=8"], "7 or 9"),
                                        (["-gcr", "-ntrks=7"], "written on 9"), (["-nrzi", "--stream"], "--stream"), (["-nrzi", "-tapread"], "-tapread"),
                                        (["-nrzi", "-ntrks=7"], "cannot carry")])
def test_cli_write_refusals(args, word, tmp_path, capfd):
    base = str(tmp_path / "t")
    open(base + ".tap", "wb").write(W.tap_image([("block", bytes(range(100, 140)))]))
    for how in ("--write=host", "--write"):
        status, _ = _cli([how] + args + [base], device=(build_emul(), NumpyBackend()))
        err = capfd.readouterr().err
        assert status == 2 and word in err and err.count("\n") == 1, err
        assert not os.path.exists(base + ".tbin")
    assert _cli(["--write=host", "-nrzi", base + ".tbin"])[0] == 2 and "SIMH .tap" in capfd.readouterr().err
    assert "--write" in cli.USAGE
