"""The amplitude shapes ON the seams of the peak path and of the dense path (tests/seam_shapes.py), on the CPU emulator, every event field against the oracle:
a plateau across a tile edge of k_sift, the two tops of a double either side of a lane strip or of the last head's split in k_sift_s, a stale minimum whose
owner lies in the tile in front, shapes around the records where k_gain_seg cuts a chain - on NRZI blocks long enough for four default segments a track, and
on GCR and PE tapes across k_dseg's sub-segments, tiles and warm-up rows.  What the row seams met is counted from the sites (coverage: samples of the shape on
both sides of the cut); what the segments met comes from the emulator's seg_shapes: line (RTFE_PREP_CHECK=2), not from this file's idea of where the count of
records began.  Only tapes the fast paths took count towards coverage (fast()).  The GPU run of the same tapes is tests/test_gpu_seam_shapes.py."""
import os

import numpy as np
import pytest

import rail_shapes as rs
import seam_shapes as ss
from emul_util import emul_frontend
from parity_util import config_for, oracle_attempts
from seam_util import (DENSE_KNOBS, DENSE_SEEDS, MIN_SEAMS, MIN_SHAPES, PATH_KNOBS, PEAK_KNOBS, PEAK_SEEDS, PHASES, ROOT,
                        dense_rows, fragments_case, ids, peak_rows, phase_case, same_results, set_knobs)



def test_seam_constants_match_the_kernels():
    """the generator aims at the seams the kernels have: a retune of a tile, a strip, a halo, the last head's split, a run, a segment, a round, a sub-segment
    or its warm-up fails here"""
    c = ss.kernel_constants(ROOT)
    assert (c["kSfStrip"], c["kPkBack"], c["kDsSub"], c["kDsJ"], c["seg_recs"]) == (ss.K_SF_STRIP, ss.K_PK_BACK, ss.K_DS_SUB, rs.K_DS_J, ss.PK_SEG_RECS)
    for k in ("sf_tile", "ds_tile", "hl", "hr", "prep_run", "window", "sfs_split", "sfs_waves", "sfs_part_strip", "sfs_part_rows", "sfs_last_head", "ds_warm", "es_round", "back", "seg_cut"):
        assert c[k], k
    assert (ss.K_SF_TILE, ss.K_DS_TILE, ss.PREP_RUN, ss.ES_ROUND, ss.K_PK_BACK) == (896, 1024, 8, 64, 64)
    assert ss.sfs_part(9) == (224, 4) and ss.sfs_part(7) == (300, 5) and ss.sfs_part(8) is None and ss.sfs_part(3) is None
    assert ss.ds_warm(13) == 48 and ss.ds_warm(20) == 56
    # the cuts are the ones rail_shapes.seams_of puts its rows next to
    for W in (13, 20):
        for c_ in range(1, 3 * ss.PREP_RUN * ss.K_SF_TILE):
            for cls in ss.cuts_of(c_, W, 9, 8) & {"sift_tile", "sift_halo", "prep_run", "dseg_sub", "dseg_tile"}:
                assert cls in ss.seams_of(c_, W) | ss.seams_of(c_ - 1, W), (c_, cls)
    assert ss.cuts_of(896, 13, 9, 8) >= {"sift_tile", "dseg_sub"} and "sift_part" in ss.cuts_of(896 + 224, 13, 9, 8) and "sift_part" not in ss.cuts_of(896 + 224, 13, 9, 3)
    assert "sift_part" in ss.cuts_of(300, 13, 7, 6) and "sift_pstrip" in ss.cuts_of(305, 13, 7, 6) and "sift_pstrip" in ss.cuts_of(4, 13, 9, 8)
    assert "dseg_warm" in ss.cuts_of(1024 - 48, 13, 9, 0) and "dseg_warm" in ss.cuts_of(128 - 8, 13, 9, 0, warm=8)


def test_the_shapes_are_what_they_say():
    """every site has samples on both sides of the cut it was aimed at; no -32768; the last head is among the heads; a plateau is flat, a double has two tops"""
    for kind, seed in (("nrzi9", 1), ("nrzi7", 3), ("gcr", 5)):
        hdr, rows0, rows, sites, opts = ss.shaped(seed, kind=kind)
        assert rows.shape[0] <= 60000 and not (rows == -32768).any() and len(sites) > 100
        assert sum(s["trk"] == hdr.ntrks - 1 for s in sites) >= 10
        for s in sites:
            if s["cut"] is not None:
                assert s["lo"] < s["cut"] <= s["hi"], s
            x = rows[s["lo"]:s["hi"] + 1, s["trk"]].astype(np.int64)
            if s["shape"] == "A-plateau":
                assert x.size >= 2 and (x == x[0]).all(), s
            if s["shape"] in ("A-double", "A-stale"):
                sg = 1 if rows0[s["row"], s["trk"]] > 0 else -1
                top = (sg * x).max()
                assert ((sg * x) >= top - 3).sum() >= 2, s
        assert (rows != rows0).any(1).sum() > 200
        k = 5
        assert (ss.phased(rows, k)[k:] == rows).all() and not ss.phased(rows, k)[:k].any()


@pytest.mark.parametrize("knobs", PEAK_KNOBS, ids=ids)
@pytest.mark.parametrize("kind", list(PEAK_SEEDS))
def test_shapes_on_the_peak_paths_seams(kind, knobs, tmp_path, monkeypatch, capfd):
    set_knobs(monkeypatch, knobs)
    monkeypatch.setenv("RTFE_PREP_CHECK", "2")
    cov, seg, nq = peak_rows(emul_frontend, kind, knobs, str(tmp_path), capfd)
    print(cov, seg)
    assert nq == len(PEAK_SEEDS[kind]), "a tape of the chosen seeds left the fast paths"
    for c in ss.SHAPES:
        assert cov.get(c, 0) >= MIN_SHAPES, (c, cov)
    for c in ss.PEAK_SEAMS + ("back_tile", "last_head"):
        assert cov.get(c, 0) >= MIN_SEAMS, (c, cov)
    # what the segments met.  planned > the chains: second segments; warm 3 is too short for a guess to come true (refused joins, and nothing for a walker to
    # adopt: re-joins need the full warm-up); a round's 64th record needs segments longer than a round
    short_warm, recs = knobs.get("RTFE_SEG_WARM") == "3", int(knobs.get("RTFE_SEG_RECS", ss.PK_SEG_RECS))
    # (back_cross - a walk back across a segment's first record - is NOT among them: at the shipped 256 records a segment, and at 32, it is met by chance only, once in
    #  the 300 tapes of profiles/seam_shapes_fuzz.txt; no knob row here exercises it, test_a_walk_back_across_a_segments_first_record forces it with 8-record segments)
    must = ["planned", "standing", "stopped", "nc_first", "nc_last", "nc_warm", "nc_near", "weak", "back_any"]
    must += ["refused"] if short_warm else (["rejoined"] if knobs.get("RTFE_SEG_REJOIN") != "0" else [])
    must += ["round_edge"] if recs > ss.ES_ROUND else []
    for k in must:
        assert seg[k] > 0, (k, seg)
    assert seg["planned"] >= 4 * (7 if kind == "nrzi7" else 9) * nq       # four segments a track and more
    if knobs.get("RTFE_SEG_REJOIN") == "0":
        assert seg["rejoined"] == 0


def test_a_walk_back_across_a_segments_first_record(tmp_path, monkeypatch, capfd):
    """the general step behind a fired record walks back to records the lean steps passed over (a stale minimum's owner lies in front of its candidate): one
    general step in a few hundred, and it crosses a segment's first record only where that record is next to it - segments of 8 records and the eight
    parameter sets of -m bring a handful per tape"""
    knobs = {"RTFE_SEG_RECS": "8"}
    set_knobs(monkeypatch, knobs)
    monkeypatch.setenv("RTFE_PREP_CHECK", "2")
    cov, seg, nq = peak_rows(emul_frontend, "nrzi9_m", knobs, str(tmp_path), capfd)
    assert nq >= 1 and seg["back_any"] > 0 and seg["back_cross"] > 0, seg


@pytest.mark.parametrize("kind", ["nrzi9", "nrzi7", "nrzi9_m", "gcr", "gcr_m", "pe"])
def test_the_shapes_change_what_the_oracle_decodes(kind, tmp_path):
    changed = 0
    for seed in (PEAK_SEEDS if kind in PEAK_SEEDS else DENSE_SEEDS)[kind]:
        hdr, rows0, rows, sites, opts = ss.shaped(seed, kind=kind)
        a = np.concatenate([x["events"] for x in oracle_attempts(hdr, rows, opts, str(tmp_path))])
        b = np.concatenate([x["events"] for x in oracle_attempts(hdr, rows0, opts, str(tmp_path))])
        changed += a.size != b.size or a.tobytes() != b.tobytes()
    assert changed >= 2, "the shapes did not change what the oracle decodes"


@pytest.mark.parametrize("kind,k", PHASES)
def test_phases_of_a_lane_strip(kind, k, tmp_path):
    """all 14 phases of a lane strip of k_sift (nine and seven tracks), and for the last head's 4-row strips in k_sift_s the phases 14 .. 17: with k mod 14 =
    0 .. 3 they pair the residues k mod 4 = 2, 3, 0, 1, which the first fourteen pair with other strip phases"""
    cov = phase_case(emul_frontend, kind, k, str(tmp_path))
    assert cov.get("sift_strip", 0) >= MIN_SEAMS and cov.get("sift_pstrip", 0) >= MIN_SEAMS, cov      # (the rare cuts were aimed at in phase 0: here their shapes lie k rows behind them)


@pytest.mark.parametrize("kind", ["nrzi9", "nrzi7"])
def test_peak_path_against_path_on_the_same_shaped_rows(kind, monkeypatch):
    hdr, rows0, rows, sites, opts = ss.shaped(PEAK_SEEDS[kind][0], kind=kind)
    same_results(emul_frontend, config_for(hdr, opts), rows, monkeypatch, [{}] + PATH_KNOBS)


@pytest.mark.parametrize("knobs", DENSE_KNOBS, ids=ids)
@pytest.mark.parametrize("kind", list(DENSE_SEEDS))
def test_shapes_on_the_dense_paths_seams(kind, knobs, tmp_path, monkeypatch):
    """GCR and PE: k_dseg's sub-segments of 128 rows, its tiles of 1024, the warm-up rows in front of a sub-segment (RTFE_DS_WARM=8: joins that fail;
    RTFE_DS_CAP=3: lists that run full).  On this path scan_stats' `parallel` is the rows k_dchain walked literally and `sequential` the events it made from
    records: the records must have done the work.  On the default row more than half of the events must come from records; the
    denominator is the oracle's events, and under -m - where the oracle's attempts are the sets it tried and the scan shares a chain among sets it cannot tell apart -
    the scan's own events with every set a chain of its own (RTFE_DENSE_DEDUP=0: dense_rows).  Measured (every tape qualifies): gcr 18 340 of 18 537 (98.9 %), pe
    17 581 of 17 859 (98.4 %), gcr -m 91 732 of 92 699 (99.0 %)."""
    set_knobs(monkeypatch, knobs)
    cov, lit, rec, ev, nq = dense_rows(emul_frontend, kind, knobs, str(tmp_path))
    print(cov, lit, rec, ev)
    assert nq == len(DENSE_SEEDS[kind]), "a tape of the chosen seeds was redone or needed an exact rescan"
    for c in ss.DENSE_SEAMS:
        assert cov.get(c, 0) >= MIN_SEAMS, (c, cov)
    for c in ss.SHAPES[:5]:
        assert cov.get(c, 0) >= MIN_SHAPES, (c, cov)
    assert rec > 0
    if not knobs:
        assert 2 * rec > ev, (rec, ev)


@pytest.mark.parametrize("kind", list(DENSE_SEEDS))
def test_dense_path_against_path_on_the_same_shaped_rows(kind, monkeypatch):
    hdr, rows0, rows, sites, opts = ss.shaped(DENSE_SEEDS[kind][0], kind=kind)
    same_results(emul_frontend, config_for(hdr, opts), rows, monkeypatch, [{}, {"RTFE_DENSE_PATH": "0"}, {"RTFE_DS_WARM": "8"}, {"RTFE_DS_CAP": "3"}])


@pytest.mark.parametrize("kind,seed", [("nrzi9", 1), ("gcr", 5)])
def test_fragments_cut_where_a_shape_lies(kind, seed):
    fragments_case(emul_frontend, kind, seed)
