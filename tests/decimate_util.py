"""The shapes at which rtfe_decimate_rows can go wrong, and one check of a call against numpy - shared by tests/test_emul_decimate.py (the kernel on the
thread emulator) and tests/test_gpu_ingest_options.py (the real one).  `call(raw, nrows_in, first, step, out, mark)` runs the entry point on host arrays
however its backend does and returns the return code; `out` ([cap, ntrks] int16) and `mark` ([1] int64) come back as the call left them."""
import numpy as np

NTRKS = (1, 7, 8, 9, 19)                                  # row bytes 2, 14, 16, 18, 38
STEPS = (1, 2, 3, 4, 7, "wide")                           # wide: more than a workgroup's span of rows
END = -32768
I64MAX = np.iinfo(np.int64).max
GUARD, PAD = 0x5A5A, 11                                   # what lies around the rows to write: a pattern, PAD rows of it in front and behind


def shapes(span_rows):
    """(ntrks, step, first, nrows_in) - span_rows(ntrks) = the raw rows a wave and a workgroup of the kernel take (rtfe_decimate_span_rows: one wave a workgroup)."""
    for ntrks in NTRKS:
        S = int(span_rows(ntrks))
        for step in STEPS:
            n = S + 3 if step == "wide" else step
            for first in sorted({0, 1, n - 1}):
                for nrows in sorted({0, first, first + 1, S - 1, S, S + 1, 3 * S + 5}):
                    yield ntrks, n, first, nrows


def mark_sets(first, step, nrows, rng):
    """Where the end marker is planted: nowhere, on a kept row, on a skipped row, in row 0, in the last row, and in two places at once."""
    out = [()]
    if nrows <= 0:
        return out
    kept = np.arange(first, nrows, step)
    skipped = np.setdiff1d(np.arange(nrows), kept)
    if kept.size:
        out.append((int(kept[kept.size // 2]),))
    if skipped.size:
        out.append((int(skipped[skipped.size // 2]),))
    out += [(0,), (nrows - 1,)]
    if nrows > 1:
        a, b = sorted(int(x) for x in rng.choice(nrows, size=2, replace=False))
        out.append((b, a))
    return out


def make_raw(ntrks, nrows, marks, rng):
    raw = rng.integers(-32767, 32768, size=(nrows, ntrks), dtype=np.int64).astype(np.int16)      # (no marker by accident)
    if ntrks > 1 and nrows:
        raw[rng.integers(0, nrows, size=min(nrows, 5)), rng.integers(1, ntrks, size=min(nrows, 5))] = END      # marker-like samples on other heads: not reported
    for m in marks:
        raw[m, 0] = END
    return raw


def check(call, ntrks, step, first, nrows, marks, rng):
    raw = make_raw(ntrks, nrows, marks, rng)
    want = raw[first::step]
    buf = np.full((PAD + want.shape[0] + PAD, ntrks), GUARD, dtype=np.uint16).view(np.int16)
    mark = np.array([12345], dtype=np.int64)
    rc, buf2, mark2 = call(raw, nrows, first, step, buf, PAD, want.shape[0], mark)
    tag = (ntrks, step, first, nrows, marks)
    assert rc == 0, tag
    assert (buf2[:PAD].view(np.uint16) == GUARD).all() and (buf2[PAD + want.shape[0]:].view(np.uint16) == GUARD).all(), tag      # nothing in front, nothing behind
    assert (buf2[PAD: PAD + want.shape[0]] == want).all(), tag
    hits = np.flatnonzero(raw[:, 0] == END)
    assert int(mark2[0]) == (int(hits[0]) if hits.size else I64MAX), tag
    assert (not marks and not hits.size) or int(hits[0]) == min(marks), tag


def check_all(call, span_rows, seed=2024):
    rng = np.random.default_rng(seed)
    n = 0
    for ntrks, step, first, nrows in shapes(span_rows):
        for marks in mark_sets(first, step, nrows, rng):
            check(call, ntrks, step, first, nrows, marks, rng)
            n += 1
    return n
