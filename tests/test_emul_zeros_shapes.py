"""-zeros and -zeros -differentiate on shaped tapes (tests/zeros_shapes.py) through the CPU emulator, end to end against the oracle: exact zeros, extremes
at the threshold code, tops that return to the same value, crossings armed for longer than a sub-segment, the rails - written on the seams of k_zeros and of
k_decode's zero-crossing mode.  The threshold ladder pins the maxvolts at which no int16 code reaches 0.2 V; the rails pin -32768 under -invert.  The GPU
run of the same checks over more seeds is tests/test_gpu_zeros_shapes.py."""
import dataclasses
import os

import numpy as np
import pytest

import zeros_shapes as zs
import zeros_util
from emul_util import emul_frontend
from readtape_amd import frontend, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bursts(hdr, rows, **kw):
    fe = emul_frontend(frontend.FrontEndConfig.from_header(hdr, find_zeros=True, **kw))
    return fe.scan(rows).fetch(events=False).bursts


def test_seam_constants_match_the_kernels():
    """the generator aims at the seams the kernels have: a retune of kZpHead / kZpSub / kZcSub or of the -zeros tile rows fails here"""
    head, sub, zc_sub, tile = zs.kernel_constants(ROOT)
    assert (head, sub, zc_sub) == (zs.KZP_HEAD, zs.KZP_SUB, zs.KZC_SUB)
    assert tile == "64 * (128 / (c->ntrks > 0 ? c->ntrks : 9))"
    assert [zs.zc_tile_rows(n) for n in (2, 7, 8, 9, 19)] == [2048, 1152, 1024, 896, 384]


def test_threshold_code_mirror():
    """zc_peak_code is the reference's comparison, code by code, in float"""
    for mv in (0.2000001, 0.2, 0.199, 2.5, 0.37, 7000.0):
        P = zs.zc_peak_code(mv)
        if P <= 32768:
            assert zs.volt(P, mv) > np.float32(0.2) and not zs.volt(P - 1, mv) > np.float32(0.2)
    assert zs.zc_peak_code(0.2000001) == 32767 and zs.zc_peak_code(0.2) == 32768 and zs.zc_peak_code(0.199) == 32769 and zs.zc_peak_code(7000.0) == 1


MODES = {"zeros": ({}, []), "diffz": ({"diff": True}, []), "invert": ({}, ["-invert"]), "skew": ({}, ["-skew=0,3,0,7,1,0,2,5,0"])}
# coverage every test's tapes must reach, counted against the shaped scans' own burst tables
MIN_SHAPES, MIN_SEAMS = 5, 3


@pytest.mark.parametrize("mode", list(MODES))
def test_shaped_zeros_against_the_oracle(mode, tmp_path):
    kw, extra = MODES[mode]
    cov, changed = {}, 0
    for seed in (1, 2, 3, 5):
        over = {"kind": "nrzi9"} if mode == "skew" else {}
        hdr, rows0, rows, sites, opts = zs.shaped(seed, _bursts, **kw, **over)
        opts = opts + extra
        msgs, b = zs.e2e(hdr, rows, opts, str(tmp_path / f"s{seed}"), emul_frontend)
        assert not msgs, f"seed {seed} {opts}: " + "\n".join(str(m) for m in msgs[:8])
        _, b0 = zs.e2e(hdr, rows0, opts, str(tmp_path / f"u{seed}"), emul_frontend)
        changed += b.size != b0.size or not np.array_equal(b["timenow_ns"], b0["timenow_ns"])
        for k, v in zs.coverage(sites, hdr, rows.shape[0], _bursts(hdr, rows)).items():
            cov[k] = cov.get(k, 0) + v
    shapes = zs.DIFF_SHAPES + ("Z-zero", "Z-flicker", "Z-rail") if kw.get("diff") else zs.SHAPES
    for c in shapes:
        assert cov.get(c, 0) >= MIN_SHAPES, (c, cov)
    for c in zs.SEAMS:
        assert cov.get(c, 0) >= MIN_SEAMS, (c, cov)
    assert changed >= 2, "the shapes did not change what the oracle decodes"


@pytest.mark.parametrize("ntrks", [2, 7, 9])
def test_shaped_zeros_path_against_path(ntrks, monkeypatch):
    """k_zeros, k_decode's parallel mode and its sequential walk, and both ends of the warm-up range, on the same shaped rows"""
    hdr, rows0, rows, sites, opts = zs.shaped(4, _bursts, ntrks=ntrks, kind="pe")
    variants = [{}, {"RTFE_ZEROS_KERNEL": "0"}, {"RTFE_ZC_PARALLEL": "0"}, {"RTFE_ZC_WARM": "16"}, {"RTFE_ZC_WARM": "64"}]
    out = zeros_util.scan_variants(lambda cfg: emul_frontend(cfg, tile_rows=zs.zc_tile_rows(ntrks)), hdr, rows, monkeypatch, variants)
    assert out[0].nbursts >= 2 and int(out[0].counts.sum()) > 100
    for r in out[1:]:
        zeros_util.same_scan(out[0], r, ntrks)
    cov = zs.coverage(sites, hdr, rows.shape[0], out[0].bursts)
    for c in ("zp_sub", "zp_warm", "zc_sub", "Z-slow", "Z-sub", "Z-edge") + (("odd_col", "unaligned_pair") if ntrks & 1 else ()):
        assert cov.get(c, 0) >= 2, (c, cov)


def _rail_tape(scale=4):
    """a clean PE tape whose samples are scaled up and clipped to the int16 range (the tape of the threshold regression)"""
    tape = synth.pe_tape(seed=5, nblocks=2, minlen=40, maxlen=80, noise_mv=0.0)
    return tape.spec.header(), np.clip(tape.rows.astype(np.int64) * scale, -32767, 32767).astype(np.int16)


def _ladder(hdr, rows, P, rng):
    """extremes of P - 2 .. P + 2 (at the int16 range's ends: clipped) written over every fourth excursion of every track"""
    rows = rows.astype(np.int64).copy()
    for t in range(rows.shape[1]):
        x = rows[:, t]
        at = np.flatnonzero(np.sign(x[1:]) * np.sign(x[:-1]) < 0) + 1
        for i, (a, b) in enumerate(zip(at[:-1], at[1:])):
            if i % 4 == 0 and b - a > 2:
                k = a + int(np.argmax(np.abs(x[a:b])))
                x[k] = np.sign(x[k]) * (P + int(rng.integers(-2, 3)))
        rows[:, t] = np.clip(x, -32768 if t else -32767, 32767)
    return rows.astype(np.int16)


@pytest.mark.parametrize("invert", [False, True], ids=["k_zeros", "k_decode"])
def test_maxvolts_where_no_code_reaches_the_threshold(invert, tmp_path):
    """maxvolts = 0.2: no int16 code is above 0.2 V, so the reference never confirms a crossing on a top.  The threshold search used to stop at 32767
    without testing it and left k_zeros (and, with -invert, k_decode) confirming crossings on full-scale samples: 4473 transitions against the oracle's 1"""
    hdr, rows = _rail_tape()
    for mv in (0.2, 0.2000001):
        h = dataclasses.replace(hdr, maxvolts=mv)
        msgs, b = zs.e2e(h, rows, ["-zeros"] + (["-invert"] if invert else []), str(tmp_path / str(mv)), emul_frontend)
        assert not msgs, "\n".join(str(m) for m in msgs[:8])
        assert (b.size < 10) if mv == 0.2 else (b.size > 4000)


@pytest.mark.parametrize("mv", [0.15, 0.199, 0.2, 0.2000001, 0.37, 7000.0])
@pytest.mark.parametrize("invert", [False, True], ids=["k_zeros", "k_decode"])
def test_threshold_ladder(mv, invert, tmp_path):
    """extremes around the threshold code where it is 1, 32767, 32768 (only -32768 reaches it) and where no code does"""
    hdr, rows = _rail_tape(scale=4 if mv < 1 else 1)
    h = dataclasses.replace(hdr, maxvolts=mv)
    P = zs.zc_peak_code(mv)
    rows = _ladder(h, rows, min(P, 32767) if P > 2 else 3, np.random.default_rng(int(mv * 1000)))
    msgs, b = zs.e2e(h, rows, ["-zeros"] + (["-invert"] if invert else []), str(tmp_path), emul_frontend)
    assert not msgs, "\n".join(str(m) for m in msgs[:8])


def inverted_rail_case(opts, tmp_path, fe_factory):
    """-invert turns a -32768 sample into +32768 (in the reference's float volts), a code no int16 holds: the zero-crossing detectors read it so.  The
    16-bit negation used to leave it at -32768 - a bottom where the reference has a top"""
    tape = synth.pe_tape(seed=5, nblocks=2, minlen=40, maxlen=80, noise_mv=0.0)
    rows = tape.rows.copy()
    for t in (3, 8):
        x = rows[:, t].astype(np.int64)
        m = np.flatnonzero((x[1:-1] < x[:-2]) & (x[1:-1] <= x[2:]) & (x[1:-1] < -5000)) + 1
        rows[m[::5], t] = -32768
    for mv in (4.4, 0.2):
        h = dataclasses.replace(tape.spec.header(), maxvolts=mv)
        msgs, b = zs.e2e(h, rows, opts, str(tmp_path / str(mv)), fe_factory)
        assert not msgs, "\n".join(str(m) for m in msgs[:8])
        assert b.size > 100 or mv == 0.2


@pytest.mark.parametrize("opts", [["-zeros", "-invert"], ["-zeros", "-invert", "-differentiate"]])
def test_inverted_negative_rail(opts, tmp_path):
    inverted_rail_case(opts, tmp_path, emul_frontend)
