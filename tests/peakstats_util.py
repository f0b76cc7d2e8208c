"""What the CPU and the GPU tests of --peakstats share: the table of command lines whose statistics files and verdict lines tests/make_peakstats_golden.py
recorded from the reference (tests/golden/peakstats_*.npz), and the comparison through readtape_amd.cli - the files byte for byte, the lines in order.

The tapes are made again from tests/cases.py / tests/cli_util.py (a golden holds the CRC of the rows it was made from); only the reference's outputs are stored."""
import io
import os
import re

import numpy as np

import cases
import cli_util
import golden_util
from readtape_amd import cli, synth

GOLDEN = golden_util.GOLDEN


def tape_flood():
    """the tape of tests/test_emul_replay.py::_event_flood_case: a confirmed crossing on almost every other row, decoded from exact rescans"""
    return synth.nrzi_tape(seed=615258906, nblocks=2, minlen=16, maxlen=200, ntrks=7, gap_samples=1500, amplitude=1.8, noise_mv=80.0, jitter=0.0)


TAPES = dict(cli_util.TAPES)
TAPES.update({"ww_skew": cases.case_ww_skew, "nrzi9_weak": cases.case_nrzi9_weak, "nrzi9_skew": cases.case_nrzi9_skew, "nrzi9_skew_long": cases.case_nrzi9_skew_long,
              "gcr_skew": cases.case_gcr_skew, "gcr_errors": cases.case_gcr_errors, "pe_drop": cases.case_pe_drop, "nrzi9_nobpi": cases.case_nrzi9_nobpi,
              "nrzi9_nobpi_skew": cases.case_nrzi9_nobpi_skew, "flood": tape_flood, "noise_only": cases.case_noise_only,
              "nrzi7_restart": cases.case_nrzi7_deskew_restart})
_made = {}


def tape(name):
    if name not in _made:
        _made[name] = TAPES[name]()
    return _made[name]


# golden name -> (tape, the command line's options); every run is `<options> g` in a directory that holds g.tbin
RUNS = {n: cli_util.RUNS[n] for n in cli_util.EXAMPLE_RUNS}
RUNS.update({
    "ww_plain": ("ww", ["-whirlwind", "-v", "-tap"]),
    "ww_skew": ("ww_skew", ["-whirlwind", "-v", "-tap", "-deskew"]),
    "weak_m": ("nrzi9_weak", ["-v", "-m", "-nrzi", "-tap"]),
    "weak_nm": ("nrzi9_weak", ["-v", "-nm", "-nrzi", "-tap"]),
    "skew_m": ("nrzi9_skew", ["-v", "-m", "-nrzi", "-tap"]),
    "skew_m_deskew": ("nrzi9_skew", ["-v", "-m", "-nrzi", "-tap", "-deskew"]),
    "skew_long": ("nrzi9_skew_long", ["-v", "-nm", "-nrzi", "-tap", "-deskew"]),
    "gcr_skew": ("gcr_skew", ["-v", "-m", "-gcr", "-tap", "-deskew"]),
    "gcr_errors": ("gcr_errors", ["-v", "-m", "-gcr", "-tap", "-correct"]),
    "pe_drop": ("pe_drop", ["-v", "-m", "-pe", "-tap"]),
    "nobpi": ("nrzi9_nobpi", ["-v", "-m", "-nrzi", "-tap"]),
    "nobpi_skew": ("nrzi9_nobpi_skew", ["-v", "-m", "-nrzi", "-tap", "-deskew"]),
    "flood": ("flood", ["-v", "-nm", "-nrzi", "-ntrks=7", "-zeros", "-differentiate", "-tap"]),
    "noise": ("noise_only", ["-v", "-m", "-nrzi", "-tap"]),
    "quiet": ("nrzi9_skew", ["-q", "-nm", "-nrzi", "-tap", "-deskew"]),
    "sub2": ("nrzi9_oversampled", ["-v", "-nm", "-nrzi", "-tap", "-subsample=2"]),
    "blk1": ("nrzi9", ["-v", "-nm", "-nrzi", "-tap", "-blklimit=1"]),
    # the first block's attempt crosses a device restart with state and is replayed a second time from an exact scan (cases.case_nrzi7_deskew_restart)
    "restart": ("nrzi7_restart", ["-v", "-nm", "-nrzi", "-ntrks=7", "-tap"]),
})
PARMS = {"restart": cases.DESKEW_RESTART_PARMS}      # golden name -> the text of g.parms beside the tape

SENTENCES = ("  the tape data head skew is minimal", "  head skew is significant; you should try again with the -deskew option")
DESKEW_SENTENCE = re.compile(r"  deskewing with delays up to -?[0-9.]+% of a bit time (seems to have been successful|wasn't entirely effective)$")
STARTS = ("  created statistics file \"", "  to graph it from Excel, open the CSV file", "  the earliest peak is ", "  that peak difference of ",
          "  the tape might have been written by two different drives", "  if so you should consider separating the data into those sections")


def is_peak_line(l):
    return l.startswith(STARTS) or l in SENTENCES or bool(DESKEW_SENTENCE.match(l))


def peak_lines(text):
    """the lines of a log that --peakstats adds: the statistics files' and the head-skew verdict's, in the log's order"""
    return [l.rstrip() for l in text.splitlines() if is_peak_line(l.rstrip())]


def other_lines(text):
    """the rest of a log, without its empty lines and the run's wall-clock time"""
    return [re.sub(r"processed in \d+ seconds \([0-9.]+ seconds/block\)", "processed in 0 seconds (0.000 seconds/block)", l.rstrip())
            for l in text.splitlines() if l.strip() and not is_peak_line(l.rstrip())]


def peak_files(wd):
    return {f: open(os.path.join(wd, f), "rb").read() for f in sorted(os.listdir(wd)) if "peakstats" in f}


def load(name):
    z = np.load(os.path.join(GOLDEN, f"peakstats_{name}.npz"))
    names = [str(n) for n in z["names"]]
    return dict(tape=str(z["tape"]), opts=[str(x) for x in z["opts"]], crc=int(z["crc"]), files={n: z[f"file{i}"].tobytes() for i, n in enumerate(names)},
                log=[str(x) for x in z["log"]])


def run_cli(name, wd, fe_factory, extra=("--peakstats",)):
    """Runs a golden's command line, with --peakstats behind its options, in the directory wd -> (status, console text)."""
    tname, opts = RUNS[name]
    os.makedirs(wd, exist_ok=True)
    tape(tname).write(os.path.join(wd, "g.tbin"))
    if name in PARMS:
        open(os.path.join(wd, "g.parms"), "w").write(PARMS[name])
    out = io.StringIO()
    status = cli.main(list(opts) + list(extra) + [os.path.join(wd, "g")], fe_factory=fe_factory, out=out)
    return status, out.getvalue()


def _log(wd):
    p = os.path.join(wd, "g.log")
    return open(p).read().replace(wd + os.sep, "") if os.path.exists(p) else ""


def check_run(name, tmp_path, fe_factory):
    """A golden's command line with --peakstats: the statistics files are the reference's, byte for byte, and so are the lines about them in the log; without
    the option nothing of it appears, and everything else the run writes is the same either way."""
    g = load(name)
    on, off = os.path.join(str(tmp_path), "on"), os.path.join(str(tmp_path), "off")
    assert cli_util.rows_crc(tape(g["tape"])) == g["crc"], "the tape is not the one the golden was made from"
    assert g["opts"] == RUNS[name][1]
    status, console = run_cli(name, on, fe_factory)
    assert status == 0, console
    got = peak_files(on)
    assert sorted(got) == sorted(g["files"]), (sorted(got), sorted(g["files"]))
    for f in g["files"]:
        assert got[f] == g["files"][f], "\n".join([f, got[f].decode(), g["files"][f].decode()])
    mine = peak_lines(_log(on))
    assert mine == g["log"], "\n".join(["got:"] + mine + ["reference:"] + g["log"])
    status, console_off = run_cli(name, off, fe_factory, extra=())
    assert status == 0, console_off
    assert not peak_files(off) and not peak_lines(_log(off)) and not peak_lines(console_off)
    assert cli_util.output_files(on) == cli_util.output_files(off)
    assert other_lines(_log(on)) == other_lines(_log(off))
    return console, _log(on)
