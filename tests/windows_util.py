"""What the CPU and the GPU tests of the windowed decode (pipeline.decode_tape_windows, ingest.decode_file_windows, the command line's --windows) share: the
cases, the span plans, and the comparison against the RESIDENT decode of the same tape with the same options - the set of output files, every file byte for
byte, the log line by line (only the elapsed seconds of the summary are normalised, as cli_util.log_lines does it), the statistics on the resident decode's keys."""
import os
import re

import numpy as np

import cases
import cli_util
from readtape_amd import pipeline
from readtape_amd.textfile import TextOptions

ELAPSED = re.compile(r"processed in \d+ seconds \([0-9.]+ seconds/block\)")      # cli_util.log_lines' normalisation
# The replay's own work counters.  With ONE fragment from the tape's first row to its end the windowed decode's replay is the resident decode's, and they are
# compared like every other key (work="equal").  With more fragments they cannot be the resident decode's: that starts the attempt behind a block where the
# block ended - often past the row up to which the burst table is proven, which costs an exact device rescan and a second delivery of its events -, a fragment
# starts its first attempt on the first row of its first burst's zone, which the table serves, and closes with an attempt that finds nothing.  There they are
# pinned to what they are made of, the sum of the fragments' own replay statistics (work = that sum); only where a block limit falls inside a journal is there
# nothing independent to hold them against (work=None).  Every other key is always compared.
WORK = ("attempts", "exact_scans", "chained", "events_delivered")


def work_sum(spans):
    return {k: sum(s[k] for s in spans) for k in WORK}


_tapes = {}


def tape(name):
    """cli_util's tapes, and tests/cases.py's by their function names"""
    if name not in _tapes:
        _tapes[name] = cli_util.tape(name) if name in cli_util.TAPES else getattr(cases, "case_" + name)()
    return _tapes[name]


def case_nrzi9_weak_long(seed=12):
    """cases.case_nrzi9_weak's recipe with seven blocks: long enough for four windows of 4096 rows"""
    from readtape_amd import synth
    return synth.nrzi_tape(seed=seed, nblocks=7, minlen=40, maxlen=80, gap_samples=1500, amplitude=0.9, amp_slope=0.12, noise_mv=60.0, jitter=0.06)


def case_pe_long(seed=15):
    """cases.case_pe's recipe with six blocks"""
    from readtape_amd import synth
    return synth.pe_tape(seed=seed, nblocks=6, minlen=30, maxlen=60, gap_samples=1500)


cases.case_nrzi9_weak_long, cases.case_pe_long = case_nrzi9_weak_long, case_pe_long

M = pipeline.DecodeOptions(multiple_tries=True)
NM = pipeline.DecodeOptions(multiple_tries=False)
# name -> (tape, decode_tape's keyword arguments; "cfgkw" holds the front end's: the resident decode takes them as arguments of their own)
CASES = {
    "labelled_bin": ("labelled", dict(opts=NM, tap_format=False, labels=True)),
    "labelled_tap": ("labelled", dict(opts=NM, tap_format=True, labels=True)),
    "flipped_h": ("flipped_h", dict(opts=NM, tap_format=False, labels=True)),
    "81_bytes": ("81_bytes", dict(opts=NM, tap_format=False, labels=True)),
    "label_parity": ("label_parity", dict(opts=NM, tap_format=False, labels=True)),
    "nrzi_weak_m": ("nrzi9_weak", dict(opts=M, tap_format=True)),
    "nrzi_weak_long_m": ("nrzi9_weak_long", dict(opts=M, tap_format=True)),
    "pe": ("pe", dict(opts=M, tap_format=True)),
    "pe_long": ("pe_long", dict(opts=M, tap_format=True)),
    "peaks_long": ("nrzi9_skew_long", dict(opts=M, tap_format=True, peakstats=True)),
    "text_linefeed_long": ("labelled", dict(opts=NM, tap_format=False, labels=True, textfile=TextOptions(None, "ascii", linefeed=True))),
    "gcr": ("gcr", dict(opts=M, tap_format=True)),
    "marks_bin": ("labelled", dict(opts=NM, tap_format=False, labels=False)),      # numbered files: .001.bin, .002.bin ...
    "text_hex_ebcdic": ("labelled", dict(opts=NM, tap_format=True, labels=True, textfile=TextOptions("hex", "ebcdic"))),
    "text_linefeed": ("nrzi9", dict(opts=M, tap_format=False, textfile=TextOptions(None, "ascii", linefeed=True))),
    "peaks": ("nrzi9_skew", dict(opts=M, tap_format=True, peakstats=True)),
    "peaks_deskew": ("nrzi9_skew_long", dict(opts=M, tap_format=True, peakstats=True, deskew=True)),
    "peaks_restart": ("nrzi7_deskew_restart", dict(opts=NM, tap_format=True, peakstats=True, parms_text=cases.DESKEW_RESTART_PARMS)),
}
PLANS = ("one", "gaps", "inside")


def grid(x):
    return int(x) // 64 * 64


def plan(t, kind):
    """the span plans of a tape on the 64-row grid: one span; a cut inside every interblock gap (every block its own fragment); cuts inside blocks (the
    ownership rule moves them)"""
    n = int(t.rows.shape[0])
    if kind == "one":
        cuts = []
    elif kind == "gaps":
        cuts = [grid((a[2] + b[1]) // 2) for a, b in zip(t.blocks[:-1], t.blocks[1:])]
    else:
        cuts = [grid((b[1] + b[2]) // 2) for b in t.blocks[1::2]]
    edges = [0] + sorted(c for c in set(cuts) if 0 < c < n) + [n]
    return list(zip(edges[:-1], edges[1:]))


def resident(name, wd, fe_factory, **more):
    """the yardstick: pipeline.decode_tape -> its statistics; the outputs are <wd>/g.*"""
    tname, kw = CASES[name] if name in CASES else name
    t = tape(tname)
    kw = dict(kw, **more)
    cfgkw = kw.pop("cfgkw", {})
    st, _ = pipeline.decode_tape(t.spec.header(), t.rows, None, log_path=os.path.join(wd, "g.log"), out_base=os.path.join(wd, "g"), in_name="g.tbin",
                                 fe_factory=fe_factory, **cfgkw, **kw)
    return st


def windows(name, wd, fe_factory, spans, **more):
    tname, kw = CASES[name] if name in CASES else name
    t = tape(tname)
    return pipeline.decode_tape_windows(t.spec.header(), t.rows, spans, log_path=os.path.join(wd, "g.log"), out_base=os.path.join(wd, "g"), in_name="g.tbin",
                                        fe_factory=fe_factory, **dict(kw, **more))


def all_log_lines(wd, name="g.log"):
    """every line of the log, the directory cut out of the file names and the elapsed seconds normalised: nothing else is dropped or rewritten"""
    text = open(os.path.join(wd, name), errors="replace").read().replace(wd + os.sep, "")
    return [ELAPSED.sub("processed in 0 seconds (0.000 seconds/block)", l.rstrip()) for l in text.splitlines()]


def peak_files(wd):
    return {f: open(os.path.join(wd, f), "rb").read() for f in sorted(os.listdir(wd)) if "peakstats" in f}


def same_value(a, b, wd_a, wd_b):
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same_value(a[k], b[k], wd_a, wd_b) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and bool(np.all(a == b))
    if isinstance(a, str) and isinstance(b, str):
        return a.replace(wd_a + os.sep, "") == b.replace(wd_b + os.sep, "")
    if isinstance(a, float) and isinstance(b, float) and a != a:
        return b != b
    return type(a) is type(b) and a == b


def compare(wd_a, st_a, wd_b, st_b, log="g.log", work="equal"):
    """wd_a / st_a: the resident decode's directory and statistics; wd_b / st_b: the windowed decode's"""
    fa, fb = cli_util.output_files(wd_a), cli_util.output_files(wd_b)
    assert sorted(fa) == sorted(fb), (sorted(fa), sorted(fb))
    for f in fa:
        assert fa[f] == fb[f], f
    pa, pb = peak_files(wd_a), peak_files(wd_b)
    assert sorted(pa) == sorted(pb), (sorted(pa), sorted(pb))
    for f in pa:
        assert pa[f] == pb[f], f
    la, lb = all_log_lines(wd_a, log), all_log_lines(wd_b, log)
    assert la == lb, "\n".join(["resident:"] + la + ["windows:"] + lb)
    if st_a is not None:
        for k in st_a:
            if k in WORK and work != "equal":
                assert work is None or st_b[k] == work[k], (k, st_b[k], work[k])
                continue
            assert k in st_b and same_value(st_a[k], st_b[k], wd_a, wd_b), (k, st_a[k], st_b.get(k))
