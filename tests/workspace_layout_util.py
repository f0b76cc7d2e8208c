"""The table tests/golden/workspace_layout.json pins: for a grid of handles, knobs and row counts, what the host API says a scan needs -
rtfe_workspace_bytes, rtfe_max_bursts, rtfe_event_capacity and whether rtfe_scan refuses the row count with -36 (the peak path's 32-bit
addressing).  Arithmetic only: nothing is allocated and no kernel runs.  Shared by tests/make_workspace_layout_golden.py (which writes the
table) and the emulated and GPU tests (which rebuild it and want it equal)."""
import contextlib
import json
import os

import cases
from parity_util import config_for

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_layout.json")

K_SF_TILE, K_DS_TILE = 896, 1024      # rtfe_device.h: kSfTile, rtfe_dense.hip: kDsTile

# name -> (tape builder of tests/cases.py - only its header is used -, oracle options, configuration keywords)
HANDLES = {
    "nrzi9":        (cases.case_nrzi9, [], {}),
    "nrzi9_m":      (cases.case_nrzi9, ["-m"], {}),
    "nrzi7":        (cases.case_nrzi7, [], {}),
    "pe_m":         (cases.case_pe, ["-m"], {}),
    "gcr_m":        (cases.case_gcr, ["-m"], {}),
    "nrzi9_zeros":  (cases.case_nrzi9, [], dict(find_zeros=True)),
    "nrzi9_diffz":  (cases.case_nrzi9, [], dict(find_zeros=True, differentiate=True)),
    "nrzi9_diffpk": (cases.case_nrzi9, [], dict(differentiate=True)),
    "nrzi9_nobpi":  (cases.case_nrzi9_nobpi_short, [], {}),
}
# one at a time, on every handle (RTFE_PEAK_PATH=1 moves PE and GCR onto the peak path; on NRZI it is the default)
KNOBS = [{}, {"RTFE_PEAK_PATH": "0"}, {"RTFE_PEAK_PATH": "1"}, {"RTFE_DENSE_PATH": "0"}, {"RTFE_CCAP": "500"}, {"RTFE_SEG_CAP": "70"},
         {"RTFE_SEG_RECS": "32"}, {"RTFE_PK_SLOT": "128"}, {"RTFE_WORK_CAP": "100"}]
# the small sizes, the seams of the peak path's and the dense path's tiles, where k_pscan's chunk count steps, long tapes, the most rows the ABI takes
ROW_COUNTS = [1, 63, 64, 65, 4095, 4096, K_SF_TILE - 1, K_SF_TILE, K_SF_TILE + 1, K_DS_TILE + 1, 1024 * K_SF_TILE + 1, 1_000_003, 50_000_000, 0x7feffff0]


@contextlib.contextmanager
def _environ(knobs):
    old = {k: os.environ.get(k) for k in knobs}
    os.environ.update(knobs)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _refuses_rows(fe, nrows):
    """rtfe_scan's argument checks alone: pointers that are not null and a workspace of any size reach the -36 check; max_bursts = 0 ends the
    call at the next one (-33) before anything is launched."""
    rc = fe.lib.rtfe_scan(fe.h, 16, nrows, nrows, 0, 1, 16, 2 ** 63, 16, 0, 16, 16, 16, 1, None)
    assert rc in (-36, -33), (rc, fe.lib.rtfe_last_error().decode())
    return rc == -36


def build_table(make_frontend):
    """{"handle|knob=value": [[workspace_bytes, max_bursts, event_capacity, refused with -36] per row count]}; make_frontend(cfg) -> FrontEnd"""
    table = {}
    for name, (build, opts, kw) in HANDLES.items():
        cfg = config_for(build().spec.header(), opts, **kw)
        for knobs in KNOBS:
            key = name + "|" + ",".join(f"{k}={v}" for k, v in knobs.items())
            with _environ(knobs):
                fe = make_frontend(cfg)
                table[key] = [[int(fe.lib.rtfe_workspace_bytes(fe.h, n)), int(fe.lib.rtfe_max_bursts(fe.h, n)), int(fe.lib.rtfe_event_capacity(fe.h, n)),
                               _refuses_rows(fe, n)] for n in ROW_COUNTS]
                fe.close()
    return table


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def differences(table, want):
    """the entries of the two tables that differ, as lines a failing test prints"""
    msgs = [f"{k}: only in the {'golden' if k in want else 'rebuilt'} table" for k in sorted(set(table) ^ set(want))]
    for k in sorted(set(table) & set(want)):
        for n, got, exp in zip(ROW_COUNTS, table[k], want[k]):
            if list(got) != list(exp):
                msgs.append(f"{k} nrows {n}: [workspace, max_bursts, event_capacity, -36] {list(got)}, golden {list(exp)}")
    return msgs
