"""Whirlwind with -zeros and / or -differentiate, end to end on the CPU (kernel sources under tests/cpu_emul): k_ww_det -> event replay ->
the Whirlwind decoder -> SIMH .tap, against the UNMODIFIED reference's .tap, block lines and event dump in the golden vectors of
tests/make_ww_detector_goldens.py.  Every field of the event dump is compared, v_avg_height included: the wide event carries the opposite
excursion the -deskew pre-pass reads."""
import ctypes as C
import os

import numpy as np
import pytest

from emul_util import emul_frontend
from golden_util import load_case
from readtape_amd import frontend, pipeline, tbin

Z_CASES = ["ww_z", "ww_z_auto", "ww_z_close", "ww_z_rough", "ww_z_unused", "ww_z_deskew"]
DZ_CASES = ["ww_dz", "ww_dz_pos", "ww_dz_rough", "ww_dz_close", "ww_dz_reverse", "ww_dz_deskew"]
DP_CASES = ["ww_dp", "ww_dp_rough"]
FAR_ZERO = "ww_dz_farzero"
WW_DETECTOR_CASES = Z_CASES + DZ_CASES + DP_CASES + [FAR_ZERO]


def decode_ww_detector_case(g, tmp_path, fe_factory, chunk_rows):
    import refdump
    o = g["oracle_opts"]
    tap = os.path.join(str(tmp_path), "out.tap")
    stats = pipeline.decode_tape_ww(g["hdr"], g["rows"], tap, log_path=tap + ".log", evt_path=tap + ".evt", fe_factory=fe_factory, chunk_rows=chunk_rows,
                                    fluxdir=next((a[9:] for a in o if a.startswith("-fluxdir=")), "neg"), reverse="-reverse" in o, deskew="-deskew" in o,
                                    find_zeros="-zeros" in o, differentiate="-differentiate" in o)
    stats["event_diffs"] = refdump.compare(refdump.load(tap + ".evt"), g["events"])          # no field ignored
    mine = [l.strip() for l in open(tap + ".log").read().splitlines() if l.startswith("wrote block") or "tapemark at" in l or "observed flux transitions" in l or "average peak height is" in l]
    assert mine == list(g["blocklog"]), (mine, list(g["blocklog"]))
    return open(tap, "rb").read(), stats


def check_case(name, chunk_rows, tmp_path, fe_factory):
    g = load_case(name)
    assert g["returncode"] == 0 and len(g["tap"]) > 0
    tap, stats = decode_ww_detector_case(g, tmp_path, fe_factory, chunk_rows)
    assert tap == g["tap"], f"{name}: .tap differs from the reference's ({len(tap)} vs {len(g['tap'])} bytes)"
    assert stats["events_delivered"] > 0 and stats["device_failures"] == 0 and stats["agc_mismatches"] == 0, stats
    assert not stats["event_diffs"], stats["event_diffs"]


@pytest.mark.parametrize("chunk_rows", [4096, 300])
@pytest.mark.parametrize("name", WW_DETECTOR_CASES)
def test_whirlwind_detectors_match_the_reference(name, chunk_rows, tmp_path):
    """-zeros, -differentiate -zeros and -differentiate on Whirlwind tapes: the reference's .tap bytes, its block lines and every field of
    its event dump, whether an attempt's rows come in one chunk or in many - both polarities, -fluxdir=auto, -reverse, unused heads, a rough
    tape, blocks a few bit times apart, -deskew (the zero detectors' state and the differentiator's last sample survive the rewind), and a
    run of exact zeros that spans a 70 000-row gap (both chunk sizes run for it too: the emulator scans its 286 400 rows in seconds)."""
    check_case(name, chunk_rows, tmp_path, emul_frontend)


def _ww_cfg(find_zeros, differentiate, nparmsets=1):
    g = load_case("ww_z")
    import dataclasses
    h = dataclasses.replace(g["hdr"], mode=tbin.MODE_WW, trkorder="", flags=g["hdr"].flags & ~tbin.FLAG_NO_REORDER)
    full = pipeline.default_parmsets(tbin.MODE_WW, 1) * nparmsets
    return frontend.FrontEndConfig.from_header(h, parmsets=pipeline.frontend_parmsets(full), find_zeros=find_zeros, differentiate=differentiate), g


@pytest.mark.parametrize("find_zeros,differentiate,kind", [(True, False, frontend.WW_ZEROS), (True, True, frontend.WW_DIFFZEROS), (False, True, frontend.WW_DIFFPEAKS)])
def test_create_accepts_the_three_detectors_and_still_refuses_two_parameter_sets(find_zeros, differentiate, kind):
    cfg, _ = _ww_cfg(find_zeros, differentiate)
    fe = emul_frontend(cfg)
    assert fe.ww_kind == kind and fe.ww_track_bytes == 432
    st = fe.ww_initial_state()
    assert len(st) == 432 * cfg.ntrks
    assert np.frombuffer(st, np.int32).reshape(cfg.ntrks, -1)[:, 0].tolist() == [kind] * cfg.ntrks
    fe.close()
    cfg2, _ = _ww_cfg(find_zeros, differentiate, nparmsets=2)
    with pytest.raises(ValueError):
        emul_frontend(cfg2)


def test_peak_detection_state_is_what_it_was():
    """rtfe_ww_initial_state, 224 bytes a track: zeros but for agc_gain = 1 and v_avg_height = 4 (the floats behind the ring and the eight ints)."""
    cfg, _ = _ww_cfg(False, False)
    fe = emul_frontend(cfg)
    assert fe.ww_kind == frontend.WW_PEAKS and fe.ww_track_bytes == 224 == fe.WW_TRACK_BYTES
    want = bytearray(224)
    want[160:168] = np.array([1.0, 4.0], np.float32).tobytes()
    assert fe.ww_initial_state() == bytes(want) * cfg.ntrks
    fe.close()


def test_a_state_of_the_wrong_kind_is_an_error_not_a_crash():
    cfg_z, g = _ww_cfg(True, False)
    cfg_dz, _ = _ww_cfg(True, True)
    cfg_pk, _ = _ww_cfg(False, False)
    fe_z, fe_dz, fe_pk = emul_frontend(cfg_z), emul_frontend(cfg_dz), emul_frontend(cfg_pk)
    rows = g["rows"]
    with pytest.raises(RuntimeError, match="bytes"):                         # a peak-detection blob (224 bytes a track) at a -zeros handle
        fe_z.ww_scan(rows, 0, 256, 0, fe_pk.ww_initial_state(), 256)
    with pytest.raises(RuntimeError, match="bytes"):                         # ... and the other way round
        fe_pk.ww_scan(rows, 0, 256, 0, fe_z.ww_initial_state(), 256)
    with pytest.raises(RuntimeError, match="another detector"):              # the right size, the other zero detector's blob
        fe_z.ww_scan(rows, 0, 256, 0, fe_dz.ww_initial_state(), 256)
    counts, events, st, flags = fe_z.ww_scan(rows, 0, 256, 0, fe_z.ww_initial_state(), 256)
    assert flags == 0 and len(st) == 432 * cfg_z.ntrks and events.dtype == frontend.WW_EVENT_DTYPE
    # the C entry points say why (rtfe_last_error): the old scan at a -zeros handle, the new one at a peak handle, a short state buffer
    lib = fe_z.lib
    buf = (C.c_ubyte * (432 * 6))()
    assert lib.rtfe_ww_detector_initial_state(fe_z.h, buf, 224 * 6) != 0 and b"bytes" in lib.rtfe_last_error()
    d_rows = fe_z._rows(rows)
    be = fe_z.backend
    scratch = be.empty(1 << 16)
    p = be.ptr(scratch)
    assert lib.rtfe_ww_scan(fe_z.h, be.ptr(d_rows), int(d_rows.shape[0]), 0, 0, 64, 0, p, p, p, p, 64, p, None) != 0
    assert b"rtfe_ww_detector_scan" in lib.rtfe_last_error()
    assert lib.rtfe_ww_detector_scan(fe_pk.h, be.ptr(d_rows), int(d_rows.shape[0]), 0, 0, 64, 0, p, p, 432 * 6, p, p, 64, p, None) != 0
    assert b"rtfe_ww_scan" in lib.rtfe_last_error()
    assert lib.rtfe_ww_detector_scan(fe_z.h, be.ptr(d_rows), int(d_rows.shape[0]), 0, 0, 64, 0, p, p, 224 * 6, p, p, 64, p, None) != 0
    assert b"bytes" in lib.rtfe_last_error()
    for fe in (fe_z, fe_dz, fe_pk):
        fe.close()


def test_decode_tape_forwards_the_detector_options(tmp_path):
    """pipeline.decode_tape on a Whirlwind header hands find_zeros / differentiate on: the bytes of decode_tape_ww with the same options
    (it used to drop both and decode with peaks)."""
    g = load_case("ww_z")
    a, b = os.path.join(str(tmp_path), "a.tap"), os.path.join(str(tmp_path), "b.tap")
    pipeline.decode_tape(g["hdr"], g["rows"], a, fe_factory=emul_frontend, find_zeros=True)
    pipeline.decode_tape_ww(g["hdr"], g["rows"], b, fe_factory=emul_frontend, find_zeros=True)
    assert open(a, "rb").read() == open(b, "rb").read() == g["tap"]
    g = load_case("ww_dz")
    pipeline.decode_tape(g["hdr"], g["rows"], a, fe_factory=emul_frontend, find_zeros=True, differentiate=True)
    assert open(a, "rb").read() == g["tap"]


def test_streaming_still_refuses_whirlwind(tmp_path):
    from readtape_amd import ingest
    g = load_case("ww_z")
    path = os.path.join(str(tmp_path), "t.tbin")
    tbin.write_tbin(path, g["hdr"], g["rows"])
    with pytest.raises(NotImplementedError):
        ingest.decode_file_streaming(path, os.path.join(str(tmp_path), "o.tap"), cfgkw=dict(find_zeros=True))
