"""CPU: ingest.plan_windows - the streaming reader's windows in used rows and the raw rows each is made of (-subsample, -skip) - and the
pre-passes' "undecided, more rows exist" switch being off by default."""
import inspect

import pytest

from readtape_amd import ingest, pipeline


def spans_before_the_options(nrows, window_rows, ramp=True):
    """The window spans as decode_file_streaming laid them out before it had -subsample and -skip (restated here: what plan_windows must reproduce)."""
    spans, lo = [], 0
    sizes = [window_rows // 4 & ~1023, window_rows // 2 & ~1023] if (ramp and window_rows >= (1 << 20) and nrows > 2 * window_rows) else []
    while lo < nrows:
        w = sizes.pop(0) if sizes else window_rows
        if ramp and not sizes and window_rows >= (1 << 20) and len(spans) >= 2 and nrows - lo <= 2 * window_rows and nrows - lo > (1 << 20):
            rest = nrows - lo
            for frac in (2, 4, 8):
                w2 = max(1 << 18, rest // frac & ~1023)
                if lo + w2 < nrows:
                    spans.append((lo, lo + w2)); lo += w2
            spans.append((lo, nrows)); lo = nrows
            break
        spans.append((lo, min(nrows, lo + w)))
        lo += w
    return spans


GRID = [(raw, win, halo, n, skip)
        for raw in (0, 1, 1023, 1024, 4097, 100_000, (1 << 20) * 7 + 12345)
        for win, halo in ((1024, 64), (4096, 1024), (1 << 14, 1 << 10), (1 << 20, 1 << 17))
        for n in (1, 2, 3, 7)
        for skip in (0, 1, 5, 1025, 200_000)]


@pytest.mark.parametrize("ramp", [True, False])
def test_every_used_row_has_one_owner_and_the_raw_spans_follow(ramp):
    for raw, win, halo, n, skip in GRID:
        plan = ingest.plan_windows(raw, win, halo, n, skip, ramp)
        used = max(0, raw - skip) // n
        tag = (raw, win, halo, n, skip)
        assert [p[0] for p in plan] == [0] * bool(plan) + [p[1] for p in plan[:-1]], tag      # contiguous from row 0: every used row in exactly one window
        assert (plan[-1][1] if plan else 0) == used, tag
        for lo, hi, raw_lo, raw_hi in plan:
            assert lo < hi and lo % 1024 == 0 and (hi % 1024 == 0 or hi == used), tag          # cuts on the grid of what the scan sees
            assert raw_lo == skip + lo * n and raw_hi == skip + min(hi + halo, used) * n, tag
            assert raw_hi <= raw, tag                                                           # nothing behind the payload
        assert [(p[0], p[1]) for p in plan] == spans_before_the_options(used, win, ramp), tag


def test_the_defaults_reproduce_the_spans_of_before():
    """subsample 1, skip 0: today's windows, the ramp at the start and at the end included."""
    seen_ramp = False
    for raw in (0, 5, 1 << 20, (1 << 21) + 1, 3 * (1 << 20) + 77, 9 * (1 << 20) + 1000, 40 * (1 << 20) + 5):
        for win in (1 << 14, 1 << 20, 1 << 22):
            for ramp in (True, False):
                plan = ingest.plan_windows(raw, win, 1 << 12, ramp=ramp)
                want = spans_before_the_options(raw, win, ramp)
                assert [(p[0], p[1]) for p in plan] == want
                assert all(p[2] == p[0] and p[3] == min(raw, p[1] + (1 << 12)) for p in plan)
                seen_ramp |= ramp and len(want) > 3 and want[0][1] == win // 4 and want[-1][1] - want[-1][0] < win // 2
    assert seen_ramp


def test_the_options_are_off_by_default():
    """The new keywords of the streaming reader, and the pre-passes' "more rows exist" switch (off: their present callers see no change)."""
    sig = inspect.signature(ingest.decode_file_streaming).parameters
    assert [sig[k].default for k in ("subsample", "skip", "deskew", "skew", "prepass_rows")] == [1, 0, False, None, 1 << 22]
    for fn in (pipeline.detect_density, pipeline.calibrate_deskew):
        assert inspect.signature(fn).parameters["more_rows"].default is False
    assert "raw" in inspect.signature(pipeline.scan_fragment).parameters
