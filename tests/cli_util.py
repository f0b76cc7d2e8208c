"""What the CPU and the GPU tests of the command line (readtape_amd/cli.py) share: the labelled tapes, the table of command lines whose outputs
tests/make_cli_golden.py recorded from the reference (tests/golden/cli_*.npz), and the comparison - file names, file bytes and log lines, byte for byte.

The tapes are made again by readtape_amd.synth (their recipes are below; a golden holds the CRC of the rows it was made from), only the reference's
outputs are stored."""
import io
import os
import re
import zlib

import numpy as np

import cases
import golden_util
import textfile_util
from readtape_amd import cli, synth

GOLDEN = golden_util.GOLDEN
ASCII_TO_EBCDIC = {}
for _code, _chars in ((0xC1, "ABCDEFGHI"), (0xD1, "JKLMNOPQR"), (0xE2, "STUVWXYZ"), (0xF0, "0123456789")):
    for _i, _ch in enumerate(_chars):
        ASCII_TO_EBCDIC[_ch] = _code + _i
ASCII_TO_EBCDIC.update({" ": 0x40, ".": 0x4B, "-": 0x60, "/": 0x61})


def ebcdic(text):
    return bytes(ASCII_TO_EBCDIC[ch] for ch in text)


def _label(text):
    assert len(text) <= 80
    return ebcdic(text.ljust(80))


def vol1(serno="TAPE01", owner="OWNER"):
    return _label("VOL1" + serno.ljust(6) + " " * 31 + owner.ljust(10))


def label1(kind, dsid, blkcnt="000000"):
    # id, dsid[17], serno[6], volseq[4], dsseq[4], genno[4], genver[2], created[6], expires[6], security, blkcnt[6], system[13]
    return _label(kind + dsid.ljust(17) + "TAPE01" + "0001" + "0001" + "    " + "  " + " 26293" + " 99365" + "0" + blkcnt + "IBM OS/VS 370")


def label2(kind):
    # id, recfm, blklen[5], reclen[5], density, dspos, job[17], recording[2], controlchar, rsvd, blkattrib
    return _label(kind + "F" + "00080" + "00080" + "3" + "0" + "JOBNAME /STEP1   " + "  " + " " + " " + "B")


def _payloads(seed, sizes):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(0, 256, size=n, dtype=np.int64).astype(np.uint8)) for n in sizes]


def _nrzi9_parity_error(payload, at):
    """the cells of a 9-track NRZI block whose word `at` has its parity bit flipped, CRC and LRC formed over the words as recorded: one parity error"""
    words = synth.nrzi_words(payload, 9)[:len(payload)]
    words[at] ^= 1
    crc = lrc = 0
    for w in words:                                           # (synth.nrzi_words' check characters, over the flipped word)
        lrc ^= w
        crc ^= w
        if crc & 2:
            crc ^= 0xF0
        lsb = crc & 1
        crc >>= 1
        if lsb:
            crc |= 0x100
    crc ^= 0x1AF
    lrc ^= crc
    words = words + [0, 0, 0, crc, 0, 0, 0, lrc]
    return ("raw", synth._words_to_transitions(words, 9), float(len(words)))


def _tape(items, seed):
    return synth.make_tape(synth.nrzi_spec(seed=seed), items, gap_samples=1500)      # 9 tracks, 800 bpi: the specs of cases.case_nrzi9


def tape_labelled(seed=71):
    """VOL1 HDR1 HDR2 * two blocks of 40 and 90 bytes * EOF1 EOF2 * | a second file whose id has five characters | * *"""
    d = _payloads(seed, (40, 90, 60))
    B, M = (lambda p: ("block", p)), ("mark",)
    return _tape([B(vol1()), B(label1("HDR1", "DOCUMENT")), B(label2("HDR2")), M, B(d[0]), B(d[1]), M, B(label1("EOF1", "DOCUMENT", "000002")), B(label2("EOF2")), M,
                  B(label1("HDR1", "NOTES")), B(label2("HDR2")), M, B(d[2]), M, B(label1("EOF1", "NOTES", "000001")), B(label2("EOF2")), M, M], seed)


def _variant(seed, second_hdr1):
    """a labelled file, then a second one whose HDR1 is `second_hdr1` (an item)"""
    d = _payloads(seed, (40, 50))
    B, M = (lambda p: ("block", p)), ("mark",)
    return _tape([B(vol1()), B(label1("HDR1", "DOCUMENT")), M, B(d[0]), M, B(label1("EOF1", "DOCUMENT", "000001")), M,
                  second_hdr1, M, B(d[1]), M, M], seed)


def tape_flipped_h(seed=72):
    """a bit flipped in the H of the second HDR1 (0xC8 -> 0xC9, "IDR1"): an ordinary block of 80 bytes, written to a numbered file"""
    lab = bytearray(label1("HDR1", "SECOND"))
    lab[0] ^= 1
    return _variant(seed, ("block", bytes(lab)))


def tape_81_bytes(seed=73):
    """a block of 81 bytes that begins HDR1: no label"""
    return _variant(seed, ("block", label1("HDR1", "SECOND") + ebcdic(" ")))


def tape_label_parity(seed=74):
    """the second HDR1 with one parity error: still a label, and "--> 1 errors" under it"""
    return _variant(seed, _nrzi9_parity_error(label1("HDR1", "SECOND"), 30))


TAPES = {"labelled": tape_labelled, "flipped_h": tape_flipped_h, "81_bytes": tape_81_bytes, "label_parity": tape_label_parity,
         "nrzi9": cases.case_nrzi9, "nrzi9_oversampled": cases.case_nrzi9_oversampled, "nrzi7_order": cases.case_nrzi7_order, "pe": cases.case_pe, "gcr": cases.case_gcr, "ww": cases.case_ww}
_made = {}


def tape(name):
    if name not in _made:
        _made[name] = TAPES[name]()
    return _made[name]


def rows_crc(t):
    return zlib.crc32(np.ascontiguousarray(t.rows).tobytes())


def _skips():
    """-skip=n with n inside the first gap and inside the first block of cases.case_nrzi9"""
    t = tape("nrzi9")
    _, first, last, _ = t.blocks[0]
    return 700, (first + last) // 2


LABEL_TAPES = ("labelled", "flipped_h", "81_bytes", "label_parity")
# golden name -> (tape, the command line's options); every run is `<options> g` in a directory that holds g.tbin
RUNS = {}
for _t in LABEL_TAPES:
    RUNS[f"{_t}_bin"] = (_t, ["-v", "-nm", "-nrzi"])
    RUNS[f"{_t}_tap"] = (_t, ["-v", "-nm", "-nrzi", "-tap"])
    RUNS[f"{_t}_nolabels"] = (_t, ["-v", "-nm", "-nrzi", "-nolabels"])
RUNS.update({
    "ex_nrzi7": ("nrzi7_order", ["-v", "-m", "-nrzi", "-ntrks=7", "-order=543210p", "-tap", "-SDS", "-linesize=144"]),      # examples/7trk_NRZI
    "ex_nrzi9": ("nrzi9", ["-v", "-m", "-nrzi", "-hex", "-ascii"]),                                                              # examples/9trk_NRZI
    "ex_pe": ("pe", ["-v", "-m", "-ntrks=9", "-pe", "-bpi=1600", "-ips=50", "-tap", "-ebcdic", "-linesize=137"]),                # examples/9trk_PE
    "ex_gcr": ("gcr", ["-v", "-m", "-gcr", "-ips=50", "-zeros", "-correct", "-tap", "-ascii", "-linefeed"]),                     # examples/9trk_GCR
    "ex_gcr_peaks": ("gcr", ["-v", "-m", "-gcr", "-ips=50", "-correct", "-tap", "-ascii", "-linefeed"]),                              # (the same on the peak detector: the synthetic tape decodes)
    "ex_ww": ("ww", ["-whirlwind", "-v3", "-fluxdir=auto", "-tap", "-deskew", "-octal2", "-flexo"]),                             # examples/6trk_Whirlwind
    "blklimit1": ("nrzi9", ["-v", "-nm", "-nrzi", "-tap", "-blklimit=1"]),
})


def _late_runs():
    gap, blk = _skips()
    return {"skip_gap": ("nrzi9", ["-v", "-nm", "-nrzi", "-tap", f"-skip={gap}"]),
            "skip_block": ("nrzi9", ["-v", "-nm", "-nrzi", "-tap", f"-skip={blk}"]),
            "skip_sub2": ("nrzi9_oversampled", ["-v", "-nm", "-nrzi", "-tap", f"-skip={gap}", "-subsample=2"])}


RUNS.update(_late_runs())
LABEL_RUNS = [n for n in RUNS if RUNS[n][0] in LABEL_TAPES]
EXAMPLE_RUNS = ["ex_nrzi7", "ex_nrzi9", "ex_pe", "ex_gcr", "ex_gcr_peaks", "ex_ww"]
OPTION_RUNS = ["blklimit1", "skip_gap", "skip_block", "skip_sub2"]


def label_lines(text):
    """the lines of a log that the label reader writes"""
    return [l.rstrip() for l in text.splitlines()
            if l.startswith("*** tape label ") or l.startswith("    volume ") or l.startswith("    block count ") or l.startswith("    job: ") or re.match(r"--> \d+ errors", l)]


def log_lines(text):
    """the lines of a log the comparison is about, in the log's order: the label reader's, golden_util.report_lines', and -blklimit's"""
    keep = set(golden_util.report_lines(text)) | set(label_lines(text))
    out = []
    for l in text.splitlines():
        l = re.sub(r"processed in \d+ seconds \([0-9.]+ seconds/block\)", "processed in 0 seconds (0.000 seconds/block)", l.rstrip())
        if l in keep or l.startswith("***blklimit="):
            out.append(l)
    return out


def output_files(wd):
    """name -> bytes of what a run left in its directory besides the input and the log; a text file without its date line"""
    files = {}
    for f in sorted(os.listdir(wd)):
        if f in ("g.tbin", "g.log") or "peakstats" in f or f.endswith(".parms"):
            continue
        data = open(os.path.join(wd, f), "rb").read()
        if f.endswith(".txt"):                                    # (its title names the file as the command line did: here with the directory)
            data = textfile_util.cut_date(data)[0].replace((wd + os.sep).encode(), b"")
        files[f] = data
    return files


def load(name):
    z = np.load(os.path.join(GOLDEN, f"cli_{name}.npz"))
    names = [str(n) for n in z["names"]]
    return dict(tape=str(z["tape"]), opts=[str(x) for x in z["opts"]], crc=int(z["crc"]), files={n: z[f"file{i}"].tobytes() for i, n in enumerate(names)},
                log=[str(x) for x in z["log"]])


def run_cli(name, wd, fe_factory, extra=()):
    """Runs a golden's command line in the directory wd -> (status, console text)."""
    tname, opts = RUNS[name]
    t = tape(tname)
    t.write(os.path.join(wd, "g.tbin"))
    out = io.StringIO()
    status = cli.main(list(opts) + list(extra) + [os.path.join(wd, "g")], fe_factory=fe_factory, out=out)
    return status, out.getvalue()


def check_run(name, tmp_path, fe_factory):
    """A golden's command line through cli.main: the files' names, their bytes and the log's lines are the reference's."""
    g = load(name)
    wd = str(tmp_path)
    assert rows_crc(tape(g["tape"])) == g["crc"], "the tape is not the one the golden was made from"
    assert g["opts"] == RUNS[name][1]
    status, console = run_cli(name, wd, fe_factory)
    assert status == 0, console
    got = output_files(wd)
    assert sorted(got) == sorted(g["files"]), (sorted(got), sorted(g["files"]))
    for f in g["files"]:
        assert got[f] == g["files"][f], f
    log = open(os.path.join(wd, "g.log")).read()
    mine = [l.replace(wd + os.sep, "") for l in log_lines(log)]
    assert mine == g["log"], "\n".join(["got:"] + mine + ["reference:"] + g["log"])
    return console, log
