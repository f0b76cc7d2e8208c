"""CPU: rtfe_decimate_rows (k_decimate, readtape_amd/csrc/rtfe_pack.hip) on the thread emulator against numpy's raw[first::step] and
np.flatnonzero(raw[:, 0] == -32768), at every shape of tests/decimate_util.py - row widths on and off the 16-byte grid, steps up to more than a
workgroup's span, windows one row short of, exactly and one row over a span - with guard rows around the output and the end marker planted on kept
and skipped rows; and every refusal the header lists."""
import ctypes as C

import numpy as np
import pytest

import decimate_util as du
from emul_util import NumpyBackend, build_emul
from readtape_amd import frontend


@pytest.fixture(scope="module")
def lib():
    return frontend._load_library(build_emul())


def _aligned(shape, lead_rows=0):
    """A zeroed [rows, ntrks] int16 array whose row `lead_rows` lies on a 16-byte boundary."""
    rows, ntrks = shape
    store = np.zeros(rows * ntrks * 2 + 32, dtype=np.uint8)
    off = -(store.ctypes.data + lead_rows * ntrks * 2) % 16
    return store[off: off + rows * ntrks * 2].view(np.int16).reshape(rows, ntrks)


def emul_call(lib):
    def call(raw, nrows, first, step, buf, pad, kept, mark):
        d_in = _aligned((max(raw.shape[0], 1), raw.shape[1]))
        d_in[: raw.shape[0]] = raw
        d_out = _aligned(buf.shape, pad)
        d_out[...] = buf
        rc = lib.rtfe_decimate_rows(d_in.ctypes.data, nrows, raw.shape[1], first, step, d_out[pad:].ctypes.data, kept, mark.ctypes.data, None)
        return rc, d_out, mark
    return call


def test_span_is_a_multiple_of_eight_rows_that_fits_the_staging_buffer(lib):
    for ntrks in range(1, frontend.MAXTRKS + 1):
        S = int(lib.rtfe_decimate_span_rows(ntrks))
        assert S >= 8 and S % 8 == 0 and S * 2 * ntrks <= 16384 < (S + 8) * 2 * ntrks
    assert lib.rtfe_decimate_span_rows(0) == 0 and lib.rtfe_decimate_span_rows(frontend.MAXTRKS + 1) == 0


def test_every_shape_against_numpy(lib):
    n = du.check_all(emul_call(lib), lib.rtfe_decimate_span_rows)
    assert n > 1000


def test_the_binding_takes_the_backends_arrays(lib):
    be = NumpyBackend()
    rng = np.random.default_rng(5)
    raw = du.make_raw(9, 2000, (1234,), rng)
    d_in, d_out, d_mark = be.rows(raw), be.rows(np.zeros((1000, 9), np.int16)), be.empty(16)
    n = frontend.decimate_rows(lib, be, d_in, 1999, 1, 2, d_out, d_mark)
    assert n == 999 and (d_out[:n] == raw[1:1999:2]).all() and not d_out[n:].any()
    assert int(be.to_numpy(d_mark, np.int64)[0]) == 1234
    with pytest.raises(RuntimeError, match="room for"):
        frontend.decimate_rows(lib, be, d_in, 2000, 0, 1, d_out, d_mark)


def test_refusals_leave_the_output_and_the_mark_alone(lib):
    ntrks = 9
    raw = du.make_raw(ntrks, 100, (3,), np.random.default_rng(1))
    d_in = _aligned(raw.shape)
    d_in[...] = raw
    d_out = _aligned((60, ntrks))
    d_out[...] = 0x5A5A
    mark = np.array([777], dtype=np.int64)
    both = _aligned((200, ntrks))                          # (for the overlap refusals: source and destination inside one buffer)
    i, o, m = d_in.ctypes.data, d_out.ctypes.data, mark.ctypes.data
    #        d_in nrows ntrks first step d_out cap mark -> code
    bad = [((None, 100, ntrks, 0, 2, o, 60, m), -1), ((i, 100, ntrks, 0, 2, None, 60, m), -1), ((i, 100, ntrks, 0, 2, o, 60, None), -1),
           ((i, 100, 0, 0, 2, o, 60, m), -3), ((i, 100, frontend.MAXTRKS + 1, 0, 2, o, 60, m), -3),
           ((i, 100, ntrks, 0, 0, o, 60, m), -34), ((i, 100, ntrks, -1, 2, o, 60, m), -34), ((i, -1, ntrks, 0, 2, o, 60, m), -34),
           ((i + 2, 98, ntrks, 0, 2, o, 60, m), -31), ((i, 100, ntrks, 0, 2, o + 2, 50, m), -31), ((i + 8, 98, ntrks, 0, 2, o, 60, m), -31),
           ((i, 100, ntrks, 0, 2, o, 49, m), -32), ((i, 100, ntrks, 1, 1, o, 60, m), -32),
           ((both.ctypes.data, 100, ntrks, 0, 2, both.ctypes.data, 200, m), -37),                                  # in place
           ((both.ctypes.data, 100, ntrks, 0, 2, both.ctypes.data + 16 * ntrks * 2 * 6, 100, m), -37),           # the output starts inside the source (row 96)
           ((both.ctypes.data + 16 * ntrks * 2, 100, ntrks, 0, 2, both.ctypes.data, 100, m), -37)]               # the source starts inside the rows to write (row 16 of 50)
    for args, code in bad:
        rc = lib.rtfe_decimate_rows(*args[:8], None)
        assert rc == code, (args, rc)
        assert lib.rtfe_last_error().decode().startswith("rtfe_decimate_rows")
        assert (d_out.view(np.uint16) == 0x5A5A).all() and int(mark[0]) == 777 and not both.any()
    # next to each other is no overlap; step 1 is a copy; zero rows to write still report the mark
    both[48: 148] = raw
    assert lib.rtfe_decimate_rows(both[48:].ctypes.data, 100, ntrks, 0, 3, both.ctypes.data, 48, m, None) == 0
    assert (both[:34] == raw[::3]).all() and not both[34: 48].any() and (both[48: 148] == raw).all() and int(mark[0]) == 3
    assert lib.rtfe_decimate_rows(i, 100, ntrks, 100, 1, o, 0, m, None) == 0 and int(mark[0]) == 3 and (d_out.view(np.uint16) == 0x5A5A).all()
    big = _aligned((100, ntrks))
    assert lib.rtfe_decimate_rows(i, 100, ntrks, 0, 1, big.ctypes.data, 100, m, None) == 0 and (big == raw).all()
    assert lib.rtfe_decimate_rows(i, 100, ntrks, 5, 1 << 62, big.ctypes.data, 1, m, None) == 0 and (big[0] == raw[5]).all() and (big[1:] == raw[1:]).all()
