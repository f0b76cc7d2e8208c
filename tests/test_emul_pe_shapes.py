"""Where a PE track's preamble ends (tests/pe_shapes.py), on the CPU emulator, every event field against the oracle: preambles of 20 .. 90 zero bits, PE tape
marks, dropouts inside a preamble, parameter sets whose t_clkwindow lies one float32 either side of the tape's own intervals, jitter, amplitude shapes on the
marker peak, the marker on k_dseg's cuts, and two start times.  Each class first asserts, from the oracle's dump alone, that its tapes contain what they were
aimed at (pe_util.assert_class: a tape that missed its aim fails), then parity with and without -m on the dense path, on k_decode (RTFE_DENSE_PATH=0), on the
peak path (RTFE_PEAK_PATH=1, and with RTFE_GAIN_FAST=0 every detection through k_gain's general step) and with RTFE_DS_LEAN=0; two scans a handle.
The emulator runs the kernels' logic, not the device's lines (fast_rcp, the packed and LDS-typed lines): tests/test_gpu_pe_shapes.py runs the same tapes there.

Mutants of the mirror these tests were tried against: profiles/README.md, section 21."""
import numpy as np
import pytest

import pe_shapes as ps
import pe_util as pu
from emul_util import emul_frontend
from parity_util import check_tape, golden_run


def test_pe_constants_match_the_kernels():
    """the generator aims at the count, the learning range, the time gates, the window's expression and the de-duplication the kernels have"""
    c = ps.kernel_constants(pu.ROOT)
    assert c["pre_count"] == ps.PRE_COUNT == 70 and c["learn"] == (ps.LEARN_FIRST, ps.LEARN_LAST) == (5, 15)
    assert c["gates"] == (ps.TIME_GATE,) * 3 and ps.TIME_GATE == 68 and ps.TIME_GATE < ps.PRE_COUNT        # (the time of peak 70 must be there when peak 71 is judged)
    assert c["clkwindow"] and c["dedup"] and c["t_peak"] and c["cf_range"]
    import seam_shapes as ss
    assert (ps.K_DS_SUB, ps.K_DS_TILE) == (128, 1024) and ss.ds_warm(13) == 48                              # (P-seam aims at these; tests/test_emul_seam_shapes.py holds them to the kernels)


def test_t_clkwindow_in_float32_and_the_ladder():
    """clkwindow() is the float32 the front end forms; cf_for() inverts it; a ladder's windows are distinct float32 values next to each other, and the text
    the oracle reads gives back the same float32 factors"""
    tp = ps.tape("P-clk", 1)
    hdr = tp["hdr"]
    assert ps.half_bit(hdr) == np.float32(np.float32(1) / np.float32(1600.0 * 50.0)) / np.float32(2)
    assert ps.clkwindow(hdr, 1.5) == np.float32(ps.half_bit(hdr) * np.float32(1.5))
    for label, t2, att, win in pu.tapes_of("P-clk", 1, m=True):
        cfs = [np.float32(p[5]) for p in t2["parmsets"]]
        assert 3 <= len(cfs) <= 8 and len(set(float(c) for c in cfs)) == len(cfs) and all(0 <= c <= 2 for c in cfs)
        assert any(c == np.float32(2.0) for c in cfs)
        # (the factor one ulp above the first may round to the first's window: two sets the de-duplication may merge, next to sets it must keep apart)
        assert [ps.clkwindow(hdr, c) for c in cfs] == win and len(set(float(w) for w in win)) >= len(win) - 1, "sets of a ladder share a window"
        w = sorted(set(float(x) for x in win))
        assert any(np.nextafter(np.float32(a), np.float32(1)) == np.float32(b) for a, b in zip(w[:-1], w[1:])), "no two windows one float32 apart"
        for c in cfs:
            assert ps.cf_for(hdr, ps.clkwindow(hdr, c)) is not None
        got = [np.float32(l.split(",")[6]) for l in t2["parms_text"].splitlines()[1:]]
        assert got == cfs
        assert len({a["parmset"] for a in att}) == len(cfs), "the reference did not try every set"


def test_the_recorded_ladder_is_the_generators():
    """tests/cases.py's pe_clk holds the parameter sets as text; they are the ladder pe_shapes draws for that tape"""
    import cases
    build = cases.CASES["pe_clk"][0]
    tp = ps.tape("P-clk", 1, nblocks=1)
    assert (build().rows == tp["rows"]).all()
    lad = ps.ladders(tp["hdr"], pu.oracle_of(tp))
    assert ps.parms_text(lad["both"]) == cases.PE_CLK_PARMS and len(lad["both"]) == 8


@pytest.mark.parametrize("cls", ps.CLASSES)
def test_tapes_are_what_they_say(cls):
    """9-track PE, at most 25 000 rows, deterministic; the options change the oracle's options only"""
    a, b = ps.tape(cls, 1), ps.tape(cls, 1)
    assert a["rows"].shape[1] == 9 and a["rows"].shape[0] <= ps.MAX_ROWS and (a["rows"] == b["rows"]).all() and a["opts"] == b["opts"]
    assert 1 <= sum("mark" not in x for x in a["meta"]) <= 5 and all(40 <= x["n"] <= 80 for x in a["meta"] if "mark" not in x)
    c = ps.tape(cls, 1, invert=True, skew=True)
    assert (c["rows"] == a["rows"]).all() and "-invert" in c["opts"] and ps.SKEW in c["opts"]
    if cls in ("P-drop", "P-shape"):
        assert (a["rows"] != a["rows0"]).any(1).sum() > 100


@pytest.mark.parametrize("m", [False, True], ids=["one_set", "m"])
@pytest.mark.parametrize("cls", ps.CLASSES)
def test_class_counters_hold_from_the_oracle_alone(cls, m):
    tot = pu.class_totals(cls, m)
    print(cls, m, tot)
    pu.assert_class(cls, tot, m)
    if cls == "P-clk":
        assert tot["sets_tried"] >= (6 if m else 1)
        # `>` against `>=`: candidates whose interval IS their set's t_clkwindow (tstart_ns = 3e12 makes the intervals float32 values: pe_shapes' docstring)
        assert tot["f32_intervals"] > 100 and tot["equal"] >= (10 if m else 1), tot
    else:
        assert tot["equal"] == 0
    if cls == "P-time":
        (_, a, atta, _), (_, b, attb, _) = pu.tapes_of(cls, 1, m)
        assert (a["rows"] == b["rows"]).all() and (a["hdr"].tstart_ns, b["hdr"].tstart_ns) == pu.TSTARTS
        ea, eb = atta[0]["events"], attb[0]["events"]
        assert ea.size == eb.size and (ea["t_peak"] != eb["t_peak"]).all()


@pytest.mark.parametrize("cls", ["P-drop", "P-shape"])
def test_the_damage_changes_what_the_oracle_decodes(cls):
    for seed in pu.SEEDS:
        (_, tp, att, _), = pu.tapes_of(cls, seed)
        clean = pu.oracle_of(dict(tp, rows=tp["rows0"]))
        a, b = np.concatenate([x["events"] for x in att]), np.concatenate([x["events"] for x in clean])
        assert a.size != b.size or a.tobytes() != b.tobytes()


@pytest.mark.parametrize("knobs", pu.PATH_KNOBS, ids=pu.ids)
@pytest.mark.parametrize("m", [False, True], ids=["one_set", "m"])
@pytest.mark.parametrize("cls", ps.CLASSES)
def test_every_event_field_against_the_oracle(cls, m, knobs, monkeypatch):
    pu.assert_class(cls, pu.class_totals(cls, m), m)
    pu.set_knobs(monkeypatch, knobs)
    assert pu.check_class(emul_frontend, cls, m) > 5000


@pytest.mark.parametrize("knobs", [{}, {"RTFE_DENSE_PATH": "0"}, {"RTFE_PEAK_PATH": "1"}], ids=pu.ids)
@pytest.mark.parametrize("opt", ["invert", "skew", "invert_skew_m"])
@pytest.mark.parametrize("cls", ps.CLASSES)
def test_the_options_of_every_class(cls, opt, knobs, monkeypatch):
    """-invert (the polarity of bit1_up) and a -skew= list"""
    kw = dict(invert="invert" in opt, skew="skew" in opt, m=opt.endswith("_m"))
    tot = pu.class_totals(cls, **kw)
    assert tot["events"] > 5000 and tot["tracks"] >= 36
    pu.set_knobs(monkeypatch, knobs)
    assert pu.check_class(emul_frontend, cls, **kw) > 5000


@pytest.mark.parametrize("cls", ps.CLASSES)
def test_path_against_path_on_the_same_rows(cls, monkeypatch):
    label, tp, att, win = pu.tapes_of(cls, 1, m=True)[0]
    pu.same_results(emul_frontend, ps.config(tp), tp["rows"], monkeypatch, pu.PATH_KNOBS + [{"RTFE_DENSE_DEDUP": "0"}])


@pytest.mark.parametrize("peak", [40, 66, 70, 71])
def test_a_fragment_cut_inside_a_preamble(peak):
    (_, tp, att, _), = pu.tapes_of("P-length", 1)
    assert pu.fragments_case(emul_frontend, tp, peak) > 5000


@pytest.mark.parametrize("knobs", [{}, {"RTFE_DENSE_PATH": "0"}, {"RTFE_PEAK_PATH": "1"}], ids=pu.ids)
@pytest.mark.parametrize("name", ["pe_pre35", "pe_pre36", "pe_pre36_invert", "pe_pre20", "pe_mark", "pe_drop", "pe_clk"])
def test_the_recorded_cases(name, knobs, tmp_path, monkeypatch):
    """the goldens of the classes (tests/cases.py) event by event; end to end they are tests/test_emul_replay.py's"""
    from golden_util import load_case
    pu.set_knobs(monkeypatch, knobs)
    g = load_case(name)
    att, cfg = golden_run(g, str(tmp_path))
    if name == "pe_clk":
        assert len(cfg.parmsets) == 8 and len({a["parmset"] for a in att}) == 8
    msgs, stats = check_tape(emul_frontend(cfg), g["hdr"], g["rows"], att)
    assert not msgs, "\n".join(msgs[:8])
    assert stats["events"] > 3000
