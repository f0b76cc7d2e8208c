"""The sharded decode of a capture FILE on CPU: two processes (torch.distributed, gloo) with the emulated kernels run shard.decode_file_sharded -
each reads its raw share of the file, thins it with rtfe_decimate_rows, rank 0 settles the density and broadcasts it, the marker all-reduce, the halo
exchange, the scans, the replays, the gather - and must write the reference's .tap (the goldens); a PE header without a density stops both."""
import dataclasses
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from readtape_amd import tbin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import os, sys, pickle
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, os.path.join(sys.argv[1], "tools"))
import torch, torch.distributed as dist
from emul_util import NumpyBackend, build_emul, emul_frontend
from readtape_amd import shard
path, out, subsample = sys.argv[2], sys.argv[3], int(sys.argv[4])
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
table, info = shard.decode_file_sharded(path, out if rank == 0 else None, rank, world, dist, subsample=subsample, halo_rows=1024, prepass_rows=4096, align=64,
                                        fe_factory=emul_frontend, _lib_path=build_emul(), _backend=NumpyBackend())
pickle.dump((table, info), open(out + f".r{rank}", "wb"))
dist.destroy_process_group()
'''


def _write(path, hdr, rows):
    with open(path, "wb") as f:
        f.write(tbin.pack_header(hdr))
        f.write(np.ascontiguousarray(rows, dtype="<i2").tobytes())
        f.write(np.array([tbin.END_MARK], dtype="<i2").tobytes())


def _two_ranks(tmp_path, hdr, rows, subsample, port, **popen):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from emul_util import build_emul
    build_emul()
    path, out, wfile = str(tmp_path / "t.tbin"), str(tmp_path / "sharded.tap"), tmp_path / "worker.py"
    _write(path, hdr, rows)
    wfile.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port + os.getpid() % 1000), WORLD_SIZE="2")
    return out, [subprocess.Popen([sys.executable, str(wfile), ROOT, path, out, str(subsample)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), **popen) for r in range(2)]


@pytest.mark.parametrize("name,subsample,port", [("nrzi9_sub2", 2, 31100), ("nrzi9_nobpi_short", 1, 32100)])
def test_two_ranks_decode_the_file_to_the_references_tap(name, subsample, port, tmp_path):
    from golden_util import load_case
    g = load_case(name)
    assert (f"-subsample={subsample}" in g["oracle_opts"]) == (subsample > 1) and (g["hdr"].bpi > 0) == (name == "nrzi9_sub2")
    out, procs = _two_ranks(tmp_path, g["hdr"], g["rows"], subsample, port)
    for p in procs:
        assert p.wait(timeout=900) == 0
    assert open(out, "rb").read() == g["tap"]
    (t0, i0), (t1, i1) = (pickle.load(open(out + f".r{r}", "rb")) for r in range(2))
    used = g["rows"].shape[0] // subsample
    assert t0 == t1 and i0 == i1 and i0["rows"] == used and i0["raw_rows"] == used * subsample and i0["bpi"] > 0
    assert [(s[0], s[1]) for s in i0["shards"]] == [(t["lo"], t["hi"]) for t in t0] and t0[1]["lo"] > 0 and t0[1]["hi"] == used
    assert sum(t["blocks"] + t["tapemarks"] for t in t0) > 0


def test_a_pe_header_without_density_stops_both_ranks(tmp_path):
    from readtape_amd import synth
    tape = synth.pe_tape(seed=5, nblocks=2)
    out, procs = _two_ranks(tmp_path, dataclasses.replace(tape.spec.header(), bpi=0.0), tape.rows, 1, 33100, stderr=subprocess.PIPE, text=True)
    errs = [p.communicate(timeout=600)[1] for p in procs]
    assert all(p.returncode != 0 for p in procs)
    assert "NRZI only" in errs[0] and "NotImplementedError" in errs[0]
    assert "another rank failed (rank 0)" in errs[1]
