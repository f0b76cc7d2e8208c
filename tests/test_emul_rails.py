"""The int16 rails through the amplitude detectors on the CPU emulator, bit-exact against the oracle: clipped tapes and single -32768 samples on the
peak path (k_sift_s / k_sift -> chains), the dense path (k_dseg -> k_dchain), the sample path (k_decode, exact rescans included) and Whirlwind's k_ww,
with and without -invert.  The reference negates the VOLTAGE (src/readtape.c:1420-1421): an inverted -32768 is +32768, volt(32768) slightly above
maxvolts - a code no int16 holds, while records, margins, packed lanes and tiles are 16 bits wide.  A burst that holds one is walked literally by k_decode
(k_rails / burst_has_rail), k_ww's ring keeps it as -32768 and reads it back; every other burst keeps its path.  On the parent of this change the
-invert cases here failed silently: 367 device events against the oracle's 662 in the first block of a clipped NRZI tape, no flag raised, the exact
rescan wrong too; k_ww answered RTFE_F_DETECTOR_FATAL.  The GPU run of the same checks is tests/test_gpu_rails.py."""
import os

import numpy as np
import pytest

import rail_shapes as rs
import refdump
from cases import CASES
from emul_util import emul_frontend
from golden_util import load_case
from parity_util import check_tape, config_for, oracle_attempts
from readtape_amd import pipeline, tbin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RAIL_CASES = sorted(n for n in CASES if "_rails" in n)
WW_RAIL_CASES = [n for n in RAIL_CASES if n.startswith("ww_")]
DIFF_RAIL_CASES = [n for n in RAIL_CASES if "diffpk" in n]             # -differentiate without -zeros: k_decode's float detector behind differentiate_tile, end to end
PEAK_RAIL_CASES = [n for n in RAIL_CASES if not n.startswith("ww_") and n not in DIFF_RAIL_CASES]
NRZI_RAIL_CASES = [n for n in PEAK_RAIL_CASES if n.startswith("nrzi")]
DENSE_RAIL_CASES = [n for n in RAIL_CASES if n.startswith(("gcr", "pe"))]
CLIPPED_CASES = ["nrzi9_rails", "gcr_rails", "pe_rails"]
NRZI_KNOBS = [{"RTFE_SIFT_GENERIC": "1"}, {"RTFE_PEAK_PATH": "0"}, {"RTFE_PEAK_PATH": "0", "RTFE_DENSE_PATH": "1"}, {"RTFE_GAIN_FAST": "0"}, {"RTFE_PK_MAR": "0"}]
DENSE_KNOBS = [{"RTFE_PEAK_PATH": "1"}, {"RTFE_DENSE_PATH": "0"}]
KNOB_NAMES = ("RTFE_SIFT_GENERIC", "RTFE_PEAK_PATH", "RTFE_DENSE_PATH", "RTFE_GAIN_FAST", "RTFE_PK_MAR")
ids = lambda k: ",".join(f"{a[5:]}={b}" for a, b in k.items()) or "default"


def set_knobs(monkeypatch, knobs):
    for k in KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def test_seam_constants_match_the_kernels():
    """the generator aims at the seams the kernels have: a retune of a tile, a halo, a segment or a run fails here"""
    c = rs.kernel_constants(ROOT)
    assert (c["kSfStrip"], c["kPkBack"], c["kChunkRows"], c["kDsSub"], c["kDsJ"], c["seg_recs"]) == (rs.K_SF_STRIP, rs.K_PK_BACK, rs.K_CHUNK_ROWS, rs.K_DS_SUB, rs.K_DS_J, rs.PK_SEG_RECS)
    for k in ("sf_tile", "ds_tile", "hl", "hr", "prep_run", "dec_tile", "window"):
        assert c[k], k
    assert (rs.K_SF_TILE, rs.K_DS_TILE, rs.PREP_RUN, rs.DEC_TILE_ROWS) == (896, 1024, 8, 512)
    assert rs.sift_halos(13) == (96, 16) and rs.sift_halos(50) == (176, 56)
    g = load_case("nrzi9_rails")
    assert rs.window(g["hdr"]) == 13 and rs.window(load_case("gcr_rails")["hdr"]) == 20 and rs.window(load_case("pe_rails")["hdr"]) == 13


def _oracle_events(hdr, rows, opts, wd):
    return rs.run_oracle(hdr, rows, opts, wd)[1]


@pytest.mark.parametrize("name", RAIL_CASES)
def test_rail_cases_hold_what_they_say(name, tmp_path):
    """the recorded tapes: -32768 on every head >= 1 (the clipped ones), never on column 0; the reference decodes them; and the rail changes what it
    decodes - the same tape stopped at -32767 gives another event stream"""
    g = load_case(name)
    rows = g["rows"]
    assert not (rows[:, 0] == -32768).any()
    on_rail = (rows == -32768).sum(0)
    if "sparse" in name:
        assert on_rail[3] >= 5 and on_rail[7] >= 5 and on_rail[1] == 1 and (rows == 32767).sum() >= 5
        k = int(np.flatnonzero(rows[:, 1] == -32768)[0])
        assert rows[k + 1, 1] == 32767 and (rows[k - 3:k, 1] == -32767).all()
    else:
        assert (on_rail[1:] >= 10).all() and ((rows == 32767).sum(0) >= 10).all(), on_rail
    ev = g["events"]
    assert g["returncode"] == 0 and ev.size > 400 and len(g["tap"]) > 50
    assert any(", ok," in l for l in g["blocklog"]) or name in DIFF_RAIL_CASES, g["blocklog"]      # (the derivative of a clipped pulse is not a pulse: that block has errors in the reference)
    a = _oracle_events(g["hdr"], rows, g["oracle_opts"], str(tmp_path / "a"))
    b = _oracle_events(g["hdr"], rs.without_rail(rows), g["oracle_opts"], str(tmp_path / "b"))
    assert not refdump.compare(a, ev)
    assert a.size != b.size or a.tobytes() != b.tobytes(), "the rail does not change what the oracle decodes"
    if name in DIFF_RAIL_CASES:                                # (there v_peak is a slope: what volt(32768) changes is the difference to its neighbours)
        return
    v = ev["v_peak"][ev["kind"] <= 1]
    top = np.float32(32768) / np.float32(32767) * np.float32(g["hdr"].maxvolts)
    if "-invert" in g["oracle_opts"]:
        assert (v == top).any() and top > np.float32(g["hdr"].maxvolts), "no transition at volt(32768)"
    else:
        assert (v == -top).any()


def sample_path(hdr):
    """do the knobs in force send this format's scans straight to k_decode (neither the peak path's nor the dense path's chains)?"""
    pk, ds = os.environ.get("RTFE_PEAK_PATH"), os.environ.get("RTFE_DENSE_PATH")
    if hdr.mode == tbin.MODE_NRZI:
        return pk == "0" and ds != "1"
    return ds == "0" and pk != "1"


def check_rails(make, hdr, rows, opts, wd, scans=2, clean=None):
    """one tape against the oracle, `scans` scans of one fresh handle (the first estimates the screen's floor from samples that span 65 535 codes, the
    others run under the floor the chains learned).  clean: no burst may be flagged or redone (the non-inverted tapes); otherwise at most the bursts
    whose rows hold a -32768 may be redone, and no other burst is flagged.  Returns the last scan's (check_tape stats, scan stats, result)."""
    os.makedirs(wd, exist_ok=True)
    att = oracle_attempts(hdr, rows, opts, wd)
    fe = make(config_for(hdr, opts))
    out = None
    for rep in range(scans):
        res = fe.scan(rows).fetch()
        st = fe.scan_stats(res)
        msgs, stats = check_tape(fe, hdr, rows, att)
        print(opts, rep, stats, {k: st[k] for k in ("bursts", "redone", "parallel", "sequential")})
        assert not msgs, f"scan {rep}: " + "\n".join(msgs[:8])
        assert stats["events"] > 0
        assert stats["speculative"] + stats["exact"] == len(att), (stats, len(att))      # (check_tape drops flagged bursts: every attempt must have been compared)
        rail = rs.rail_bursts(rows, res.bursts[:res.nbursts])
        if clean if clean is not None else "-invert" not in opts:
            assert st["redone"] == 0 and stats["flags"] == 0, (st["redone"], stats["flags"])
        else:
            # the scan publishes no per-burst "redone" (only the count), so the count is pinned from both sides: under -invert EVERY burst that holds a
            # -32768 leaves its chains (k_rails) - were one burst without such a sample redone as well, the count would exceed theirs.  The sample path
            # (no chains: k_decode takes every burst) counts none.
            n_rail = int(rail.sum())
            if "-invert" in opts and not sample_path(hdr):
                assert st["redone"] == n_rail, (st["redone"], rail)
            else:
                assert st["redone"] <= n_rail, (st["redone"], rail)
            assert (res.bursts["flags"][:res.nbursts][~rail] == 0).all(), (res.bursts["flags"], rail)
        out = (stats, st, res)
    return out


@pytest.mark.parametrize("name", PEAK_RAIL_CASES)
def test_rail_cases_against_the_oracle(name, tmp_path):
    g = load_case(name)
    stats, st, res = check_rails(emul_frontend, g["hdr"], g["rows"], g["oracle_opts"], str(tmp_path))
    if "sparse" in name:                                       # the bursts of the blocks are apart: only those that hold a site leave their chains
        rail = rs.rail_bursts(g["rows"], res.bursts[:res.nbursts])
        assert 0 < rail.sum() and st["redone"] == rail.sum()


@pytest.mark.parametrize("knobs", NRZI_KNOBS, ids=ids)
@pytest.mark.parametrize("name", NRZI_RAIL_CASES)
def test_nrzi_rail_cases_on_every_path(name, knobs, tmp_path, monkeypatch):
    set_knobs(monkeypatch, knobs)
    g = load_case(name)
    check_rails(emul_frontend, g["hdr"], g["rows"], g["oracle_opts"], str(tmp_path))


@pytest.mark.parametrize("knobs", DENSE_KNOBS, ids=ids)
@pytest.mark.parametrize("name", DENSE_RAIL_CASES)
def test_gcr_pe_rail_cases_on_every_path(name, knobs, tmp_path, monkeypatch):
    set_knobs(monkeypatch, knobs)
    g = load_case(name)
    check_rails(emul_frontend, g["hdr"], g["rows"], g["oracle_opts"], str(tmp_path))


def same_results(make, hdr, rows, opts, monkeypatch, variants):
    """one scan per knob set: the same burst table and, per (burst, parameter set, track), the same events byte for byte - also where no oracle attempt looks"""
    cfg = config_for(hdr, opts)
    out = []
    for knobs in variants:
        set_knobs(monkeypatch, knobs)
        out.append(make(cfg).scan(rows).fetch())
    r0 = out[0]
    assert r0.nbursts > 0 and int(r0.counts.sum()) > 100
    for knobs, r in zip(variants[1:], out[1:]):
        assert r.nbursts == r0.nbursts, knobs
        for k in ("zone_first", "zone_end", "reset_sample", "safe_last", "end_sample", "flags"):
            assert (r.bursts[k][:r.nbursts] == r0.bursts[k][:r0.nbursts]).all(), (knobs, k)
        for b in range(r0.nbursts):
            for p in range(len(cfg.parmsets)):
                for t in range(cfg.ntrks):
                    assert r.track_events(b, p, t).tobytes() == r0.track_events(b, p, t).tobytes(), (knobs, b, p, t)


@pytest.mark.parametrize("name", PEAK_RAIL_CASES)
def test_rail_cases_path_against_path(name, monkeypatch):
    g = load_case(name)
    same_results(emul_frontend, g["hdr"], g["rows"], g["oracle_opts"], monkeypatch, [{}] + (NRZI_KNOBS if name.startswith("nrzi") else DENSE_KNOBS))


def decode_rail_case(g, tmp_path, fe_factory, chunk_rows=4096):
    """the whole pipeline on a recorded case: (.tap bytes, differences between the transitions the decoders were handed and the reference's)"""
    o = g["oracle_opts"]
    tap = os.path.join(str(tmp_path), "out.tap")
    if g["hdr"].mode == tbin.MODE_WW:
        pipeline.decode_tape_ww(g["hdr"], g["rows"], tap, log_path=tap + ".log", evt_path=tap + ".evt", fe_factory=fe_factory, chunk_rows=chunk_rows, invert="-invert" in o,
                                fluxdir=next((a[9:] for a in o if a.startswith("-fluxdir=")), "neg"))
    else:
        pipeline.decode_tape(g["hdr"], g["rows"], tap, log_path=tap + ".log", evt_path=tap + ".evt", fe_factory=fe_factory, invert="-invert" in o,
                             differentiate="-differentiate" in o, opts=pipeline.DecodeOptions(multiple_tries="-m" in o), skew=next(([int(x) for x in a[6:].split(",")] for a in o if a.startswith("-skew=")), None))
    mine = [l.strip() for l in open(tap + ".log").read().splitlines() if l.startswith("wrote block") or "tapemark at" in l or "observed flux transitions" in l or "density was set to" in l or "average peak height is" in l]
    assert mine == list(g["blocklog"]), (mine, list(g["blocklog"]))
    return open(tap, "rb").read(), refdump.compare(refdump.load(tap + ".evt"), g["events"])


@pytest.mark.parametrize("name", PEAK_RAIL_CASES + DIFF_RAIL_CASES)
def test_rail_cases_tap_bytes_match_the_reference(name, tmp_path):
    g = load_case(name)
    tap, diffs = decode_rail_case(g, tmp_path, emul_frontend)
    assert tap == g["tap"] and not diffs, diffs


@pytest.mark.parametrize("chunk_rows", [4096, 300])
@pytest.mark.parametrize("name", WW_RAIL_CASES)
def test_whirlwind_rail_cases_tap_bytes_match_the_reference(name, chunk_rows, tmp_path):
    """k_ww's ring holds the inverted -32768: the window's maximum is a value the ring used not to contain (RTFE_F_DETECTOR_FATAL on the parent)"""
    g = load_case(name)
    tap, diffs = decode_rail_case(g, tmp_path, emul_frontend, chunk_rows)
    assert tap == g["tap"] and not diffs, diffs


LADDER_CASES = [(n, mv, inv) for n in ("nrzi9", "gcr", "pe") for mv in rs.LADDER for inv in (False, True)]


def ladder_case(make, name, mv, invert, wd):
    """a clean tape digitised again at `mv` volts full scale: 6 - 11 % of the samples on the rails at 1.5 V, peaks of some 250 codes at 400 V"""
    hdr0, rows0, opts0, _ = rs.base_tape(name, 21)
    hdr, rows = rs.rescaled(hdr0, rows0, mv)
    if mv < 2.5 and not (name == "gcr" and mv > 2):            # (the GCR tape's pulses are 1.8 - 2.2 V: 2.2 V full scale clips none of them)
        assert (rows[:, 1:] == -32768).any(0).all() and 0.03 < np.mean(np.abs(rows.astype(np.int32)) >= 32767) < 0.15
    else:
        assert np.abs(rows.astype(np.int32)).max() < 32767 * 4.4 / mv * 1.1
    opts = ["-invert"] if invert else []
    check_rails(make, hdr, rows, opts, wd, scans=1)
    if name == "nrzi9" and invert:
        check_rails(make, hdr, rows, opts + ["-m"], wd, scans=1)


@pytest.mark.parametrize("name,mv,invert", LADDER_CASES)
def test_full_scale_ladder(name, mv, invert, tmp_path):
    ladder_case(emul_frontend, name, mv, invert, str(tmp_path))


SHAPED_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)


def shaped_case(make, seed, wd, over=None):
    """tape `seed` of tests/rail_shapes.py against the oracle (Whirlwind: end to end; the others: every event field, then end to end); returns its coverage"""
    d = dict(rs.draw(seed), **(over or {}))
    hdr, rows, sites, opts, blocks = rs.shaped(seed, **(over or {}))
    assert not (rows[:, 0] == -32768).any() and (rows[:, 1:] == -32768).any(0).all(), "a head without a -32768"
    W = rs.window(hdr) if hdr.mode != tbin.MODE_WW else 8
    cov = rs.coverage(rows, sites, W)
    if d["how"] == "sparse":
        for c in rs.SHAPES:
            assert cov.get(c, 0) >= 1 or (c == "R-skew" and not d["skew"]), (c, cov)
        for c in rs.SEAMS:
            assert cov.get(c, 0) >= 1 or (c == "gain_seg" and not d["kind"].startswith("nrzi")), (c, cov)      # (k_gain_seg serves NRZI: only its tapes have a block of several segments)
    a = _oracle_events(hdr, rows, opts, os.path.join(wd, "a"))
    b = _oracle_events(hdr, rs.without_rail(rows), opts, os.path.join(wd, "b"))
    assert a.size > 300 and (a.size != b.size or a.tobytes() != b.tobytes()), "the rail does not change what the oracle decodes"
    if hdr.mode != tbin.MODE_WW:
        # (a sparse tape's lone -32768 in a gap is a burst of its own with no room for a safe restart: flagged and redone with or without -invert)
        stats, st, res = check_rails(make, hdr, rows, opts, os.path.join(wd, "c"), clean=d["how"] != "sparse" and not d["invert"])
        if d["how"] == "sparse":
            rail = rs.rail_bursts(rows, res.bursts[:res.nbursts])
            assert not rail.all(), "no burst without a -32768: nothing shows that such bursts keep their path"
    for chunk in ((4096, 300) if hdr.mode == tbin.MODE_WW else (4096,)):
        msgs, _ = rs.e2e(hdr, rows, opts, os.path.join(wd, f"e{chunk}"), make, chunk_rows=chunk)
        assert not msgs, f"seed {seed} {d} {opts}: " + "\n".join(str(m) for m in msgs[:8])
    return d, cov


@pytest.mark.parametrize("seed", SHAPED_SEEDS)
def test_shaped_rails_against_the_oracle(seed, tmp_path):
    shaped_case(emul_frontend, seed, str(tmp_path))


@pytest.mark.parametrize("kind", rs.KINDS)
@pytest.mark.parametrize("how", ["sparse", "x2"])
def test_shaped_rails_of_every_kind_inverted(kind, how, tmp_path):
    """what the seeds' draw may miss: every format, sparse and clipped, under -invert; NRZI-9 with deskew delays, Whirlwind with -fluxdir=auto"""
    over = dict(kind=kind, how=how, invert=True, skew=kind == "nrzi9", m=False, fluxdir="auto" if kind == "ww" else None)
    shaped_case(emul_frontend, 11, str(tmp_path), over)


def test_the_seeds_cover_formats_and_modes():
    ds = [rs.draw(s) for s in SHAPED_SEEDS]
    assert len({d["kind"] for d in ds}) >= 3 and {d["how"] == "sparse" for d in ds} == {True, False} and {d["invert"] for d in ds} == {True, False}
