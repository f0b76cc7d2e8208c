"""The amplitude shapes on the seams of the peak path and of the dense path on the MI355X: the tapes of tests/test_emul_seam_shapes.py through the C ABI,
every event field against the oracle, path against path byte for byte, as fragments, through the streaming reader's windows, and replayed from a captured
graph.  The device cannot print what its segments met: only the seeds whose coverage the emulator test asserts run here, and every tape must have been
taken by the fast paths (nothing redone, no chain gave up, no exact rescan, the lean step more than twice the general step's share).  The packed
k_sift_s - the last head's split among it - is code the emulator does not run: these tests are what sees it."""
import numpy as np
import pytest

import seam_shapes as ss
from parity_util import config_for
from readtape_amd import frontend
from seam_util import (DENSE_KNOBS, DENSE_SEEDS, MIN_SEAMS, MIN_SHAPES, PATH_KNOBS, PEAK_KNOBS, PEAK_SEEDS, PHASES, dense_rows, fragment_cuts, fragments_case, ids, peak_rows,
                       phase_case, same_results, set_knobs)

pytestmark = pytest.mark.gpu


def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return frontend.FrontEnd


@pytest.mark.parametrize("knobs", PEAK_KNOBS + [{"RTFE_SEG_RECS": "8"}], ids=ids)
@pytest.mark.parametrize("kind", list(PEAK_SEEDS))
def test_shapes_on_the_peak_paths_seams(kind, knobs, tmp_path, monkeypatch):
    set_knobs(monkeypatch, knobs)
    cov, seg, nq = peak_rows(_gpu(), kind, knobs, str(tmp_path))
    assert nq == len(PEAK_SEEDS[kind]), "a tape left the fast paths"
    for c in ss.SHAPES:
        assert cov.get(c, 0) >= MIN_SHAPES, (c, cov)
    for c in ss.PEAK_SEAMS + ("back_tile", "last_head"):
        assert cov.get(c, 0) >= MIN_SEAMS, (c, cov)


@pytest.mark.parametrize("kind,k", PHASES)
def test_phases_of_a_lane_strip(kind, k, tmp_path):
    cov = phase_case(_gpu(), kind, k, str(tmp_path))
    assert cov.get("sift_strip", 0) >= MIN_SEAMS and cov.get("sift_pstrip", 0) >= MIN_SEAMS, cov


@pytest.mark.parametrize("kind", ["nrzi9", "nrzi7", "nrzi9_m"])
def test_peak_path_against_path_on_the_same_shaped_rows(kind, monkeypatch):
    hdr, rows0, rows, sites, opts = ss.shaped(PEAK_SEEDS[kind][0], kind=kind)
    same_results(_gpu(), config_for(hdr, opts), rows, monkeypatch, [{}] + PATH_KNOBS + [{"RTFE_SIFT_PLAIN": "0"}])


@pytest.mark.parametrize("knobs", DENSE_KNOBS, ids=ids)
@pytest.mark.parametrize("kind", list(DENSE_SEEDS))
def test_shapes_on_the_dense_paths_seams(kind, knobs, tmp_path, monkeypatch):
    set_knobs(monkeypatch, knobs)
    cov, lit, rec, ev, nq = dense_rows(_gpu(), kind, knobs, str(tmp_path))
    assert nq == len(DENSE_SEEDS[kind]), "a tape was redone or needed an exact rescan"
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
    same_results(_gpu(), config_for(hdr, opts), rows, monkeypatch, [{}, {"RTFE_DENSE_PATH": "0"}, {"RTFE_DS_WARM": "8"}, {"RTFE_DS_CAP": "3"}])


@pytest.mark.parametrize("kind,seed", [("nrzi9", 1), ("nrzi7", 3), ("gcr", 5), ("pe", 5)])
def test_fragments_cut_where_a_shape_lies(kind, seed):
    fragments_case(_gpu(), kind, seed)


@pytest.mark.parametrize("kind,seed", [("nrzi9", 1), ("nrzi7", 3), ("nrzi9_m", 1), ("pe", 5), ("pe", 6)])
def test_shaped_seam_on_a_streamed_windows_edge(kind, seed, tmp_path):
    """the streaming reader's windows cut where a shape lies (every window edge a multiple of the first, itself a multiple of 1024 that a site straddles),
    halos shorter than the block (they have to grow): the .tap of the whole-tape decode, whose events the tests above hold against the oracle.  No GCR here: a
    GCR block with one of these shapes in it is unusable in the reference too ("tracks mismatched"), its .tap is empty and the comparison would say nothing - GCR's
    events across the same cuts are test_fragments_cut_where_a_shape_lies'."""
    from readtape_amd import ingest, pipeline, tbin
    _gpu()
    hdr, rows0, rows, sites, opts = ss.shaped(seed, kind=kind)
    cuts = fragment_cuts(sites, 4096, rows.shape[0] // 3, n=1)
    assert cuts, "no site across a multiple of 1024"
    pipeline.decode_tape(hdr, rows, str(tmp_path / "whole.tap"), opts=pipeline.DecodeOptions(multiple_tries="-m" in opts))
    want = open(tmp_path / "whole.tap", "rb").read()
    path = str(tmp_path / "t.tbin")
    tbin.write_tbin(path, hdr, rows)
    st = ingest.decode_file_streaming(path, str(tmp_path / "s.tap"), window_rows=cuts[0], halo_rows=1 << 10, replay_threads=4, replay_split=3, opts=pipeline.DecodeOptions(multiple_tries="-m" in opts))
    assert len(want) > 250, "the tape decodes to next to nothing: the comparison would be vacuous"
    assert open(tmp_path / "s.tap", "rb").read() == want
    assert st["rows"] == rows.shape[0] and st["windows"] >= 3


@pytest.mark.parametrize("kind,seed", [("nrzi9", 2), ("nrzi9_m", 1), ("gcr_m", 6)])
def test_graph_replayed_scans_of_a_shaped_tape(kind, seed):
    """rtfe_set_graphs: the same buffers scanned twice (a capture and a replay) leave what the direct launches leave"""
    import torch
    make = _gpu()
    hdr, rows0, rows, sites, opts = ss.shaped(seed, kind=kind)
    cfg = config_for(hdr, opts)

    def lists(r):
        r.fetch()
        return r.nbursts, r.bursts.tobytes(), {(b, p, t): r.track_events(b, p, t).tobytes() for b in range(r.nbursts) for p in range(len(cfg.parmsets)) for t in range(cfg.ntrks)}
    want = lists(make(cfg).scan(rows))
    assert want[0] > 0 and sum(len(v) for v in want[2].values()) > 1000
    fe = make(cfg)
    fe.set_graphs(True)
    st = torch.cuda.Stream()
    d_rows = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    with torch.cuda.stream(st):
        for i in range(2):
            assert lists(fe.scan(d_rows, stream=st.cuda_stream)) == want, i
    st.synchronize()
