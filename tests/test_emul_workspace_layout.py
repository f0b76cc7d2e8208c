"""The workspace layout against tests/golden/workspace_layout.json (recorded before the layout became one function): every size the host API
reports, for the handles, knobs and row counts of tests/workspace_layout_util.py, through the CPU emulator's one CU.  An interior region
whose size changes moves the total at most of the row counts; a 256-byte alignment cannot hide it at all of them."""
import workspace_layout_util as wl
from emul_util import NumpyBackend, build_emul
from readtape_amd import frontend


def test_emulated_workspace_layout_is_the_recorded_one():
    gold = wl.load_golden()
    assert gold["row_counts"] == wl.ROW_COUNTS and gold["emul"]["num_cus"] == 1
    lib = build_emul()
    table = wl.build_table(lambda cfg: frontend.FrontEnd(cfg, _lib_path=lib, _backend=NumpyBackend()))
    assert len(table) == len(wl.HANDLES) * len(wl.KNOBS)
    msgs = wl.differences(table, gold["emul"]["table"])
    assert not msgs, f"{len(msgs)} entries differ\n" + "\n".join(msgs[:20])
