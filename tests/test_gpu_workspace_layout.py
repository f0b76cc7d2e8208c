"""The workspace layout on the device against the "gpu" table of tests/golden/workspace_layout.json: the deferred candidates' capacity depends
on the CU count, which the emulator's table (one CU) cannot pin.  The table holds for the device it was recorded on: another CU count fails."""
import pytest

import workspace_layout_util as wl
from readtape_amd import frontend

pytestmark = pytest.mark.gpu


def test_workspace_layout_is_the_recorded_one():
    import torch
    gold = wl.load_golden()
    assert gold["row_counts"] == wl.ROW_COUNTS
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert cus == gold["gpu"]["num_cus"], f"this device has {cus} CUs, the table was recorded on one with {gold['gpu']['num_cus']}: record it again (tests/make_workspace_layout_golden.py --gpu)"
    table = wl.build_table(frontend.FrontEnd)
    assert len(table) == len(wl.HANDLES) * len(wl.KNOBS)
    msgs = wl.differences(table, gold["gpu"]["table"])
    assert not msgs, f"{len(msgs)} entries differ\n" + "\n".join(msgs[:20])
