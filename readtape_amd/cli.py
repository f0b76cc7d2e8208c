"""The command line: `python -m readtape_amd <options> <basefilename>[.ext]`, the reference's `readtape <options> <basefilename>`.

The option grammar is the reference's (src/readtape.c:816-1033): options are the arguments that begin with '-', up to the first one that does not;
keywords match in any letter case and as the whole argument; their order matters where it matters there (-gcr sets the speed, -whirlwind the density
and -nm, -octal2 the data spacing, -skew= needs -ntrks= in front of it, -order= is a Whirlwind role string only behind -whirlwind).  What is found
for the base name, and which header field or option wins, follows src/readtape.c:1955-1984, 1586-1596 and 1330-1355.

  main(argv, fe_factory=None, out=None) -> exit status    0 decoded ("ok" or "bad"), 1 usage asked for, 2 an option that is parsed but not built,
                                                           4 no base name, 99 a bad option or a condition that is fatal in the reference
  parse_args(argv) -> (Options, the arguments behind the options)
  find_parms(base, mode) / parms_options(text)             the parameter-set file of a run and the `readtape` lines in it

One decode is one call of pipeline.decode_tape (ingest.decode_file_streaming with --stream, textfile.write_text[_device] with -tapread); a list run
(-f) decodes its files one after the other in this process.  --write goes the other way: tapewrite.write_tbin[_device] renders a .tap image as a .tbin."""
from __future__ import annotations

import dataclasses
import os
import re
import sys
import tempfile
from dataclasses import dataclass

import numpy as np

from . import tbin

MINTRKS, MAXTRKS, MAXLINE = 5, 19, 400                      # src/decoder.h:90, src/csvtbin.h:29, src/decoder.h:95
INT_MAX = 0x7fffffff
DEVICE_TEXT_BYTES = 64 << 20                               # -tapread: images of this size and more are formatted on the device
MODE_NAMES = {tbin.MODE_PE: "PE", tbin.MODE_NRZI: "NRZI", tbin.MODE_GCR: "GCR", tbin.MODE_WW: "Whirlwind"}      # modename(), src/readtape.c:1113

USAGE = """\
readtape_amd: a decoder for digitized analog magnetic tape data (HIP front end, gfx950)

use: python -m readtape_amd <options> <basefilename>[.ext]

  The input file is <basefilename> with .csv, .tbin, or .tap,
    which may optionally be included in the command.
   If the extension is not specified, it tries .csv first
    then .tbin, and .tap only if -tapread is specified.
  A .csv file is converted as csvtbin converts it (with its defaults) and the
    result is decoded: the run equals csvtbin followed by readtape, not
    readtape's own reading of the floating point samples.

  The output files will be <basefilename>.xxx by default.

  The optional parameter file is <basefilename>.parms,
   or NRZI,PE,GCR,Whirlwind.parms, in the base or current directory.

options:
  -ntrks=n       set the number of tracks to n
  -order=        set input data order for tracks 0..ntrks-2,P, where 0=MSB
                 default: 01234567P for 9 trk, 012345P for 7 trk
                 (for Whirlwind: a combination of C L M c l m and x's)
  -pe            PE (phase encoding)
  -nrzi          NRZI (non return to zero inverted)
  -gcr           GCR (group coded recording)
  -whirlwind     Whirlwind I 6-track 2-bit-per-character
  -ips=n         speed in inches/sec (default: 50, except 25 for GCR)
  -bpi=n         density in bits/inch (default: autodetect)
  -zeros         base decoding on zero crossings instead of peaks
  -differentiate do simple delta differentiation of the input data
  -even          expect even parity instead of odd (for 7-track NRZI BCD tapes)
  -revparity=n   reverse parity for blocks up to n bytes long
  -invert        invert the data so positive peaks are negative and vice versa
  -fluxdir=d     flux direction is 'pos', 'neg', or 'auto' for each block
  -reverse       reverse bits in a word and words in a block (Whirlwind only)
  -skip=n        skip the first n samples
  -blklimit=n    stop after n blocks
  -subsample=n   use only every nth data sample
  -tap           create one SIMH .tap file from all the data
  -deskew        do NRZI track deskewing based on the beginning data
  -skew=n,n      use this skew, in #samples for each track, rather than deducing it
  -correct       do error correction, where feasible
  -addparity     include the parity bit as the highest bit in the data (for ntrks<9)
  -tbin          only look for a .tbin input file, not .csv first
  -nolog         don't create a log file
  -nolabels      don't try to decode IBM standard tape labels
  -textfile      create an interpreted .<options>.txt file from the data
                   numeric options: -hex -octal (bytes) -octal2 (16-bit words)
                   character options: -ASCII -EBCDIC -BCD -sixbit -B5500 -SDS -SDSM
                        -flexo -adage -adagetape -CDC -Univac
                   characters per line: -linesize=nn
                   space every n bytes of data: -dataspace=n
                   make LF or CR start a new line: -linefeed
  -tapread       read a SIMH .tap file to produce a textfile; the input may have any extension
  -outf=bbb      use bbb as the <basefilename> for output files
  -outp=ppp      otherwise use ppp as an optional prepended path for output files
  -m             try multiple ways to decode a block (the default unless Whirlwind)
  -nm            don't try multiple ways to decode a block
  -v[n]          verbose mode [level n, default is 1; higher levels add nothing]
  -q             quiet mode (only say "ok" or "bad")
  -f             take a file list from <basefilename>.txt; -outf= names the output of every
                 file of the list, otherwise each file's own name follows -outp=
  --stream       decode a .tbin through device windows instead of reading it whole
                 (needs -tap and -nolabels; not for Whirlwind, -textfile or -blklimit; no log)
  --windows[=n]  decode a .tbin through device windows [of n rows] with everything the whole-file
                 decode writes: the log, labels and label-named files, numbered .bin files,
                 -textfile, -blklimit, -order/-bpi/-ips, --peakstats (not for Whirlwind, a .csv
                 input, or together with --stream)
  --peakstats    write <basefilename>.peakstats.csv (and, with -deskew, .peakstats_deskew.csv):
                 per track, where the flux transitions fall against the decoder's clock; and
                 say under the summary whether the head skew is significant (-q: only the
                 -deskew file, as in readtape; every file of a -f list gets its own; not with
                 --stream, whose windows do not share the bins the first transition fixes)
  --write[=host] the other direction: render the SIMH file <basefilename>[.tap] as the analog
                 <basefilename>.tbin a head would have read, on the device [=host: on the host,
                 the same bytes].  Give the format: -nrzi (-ntrks=7 or 9, -even), -pe or -gcr;
                 -bpi= -ips= -outf= -outp= as above; --tdelta=ns the sample time, --noise=mV,
                 --jitter=cells, --seed=n, --gap=samples between blocks.  Whirlwind is not written.

not built (the run ends with status 2): -showibg=n -sumt=sss -sumc=ccc -adjskew -d[n]
  <basefilename>.peakstats.csv is not written unless --peakstats is given: gathering it puts
  a histogram update on every flux transition of every attempt of the host replay, which
  then takes 1.05 times as long (an NRZI tape, one parameter set; profiles/peakstats.txt).
"""


class CliExit(Exception):
    """The run ends here with this status; `message` goes to stderr (usage=True: the usage text follows it)."""

    def __init__(self, status, message="", usage=False):
        super().__init__(message)
        self.status, self.message, self.usage = status, message, usage


def fatal(msg):
    return CliExit(99, f"\n***FATAL ERROR: {msg}\n")


@dataclass
class Options:
    """The state the reference keeps in its globals while it reads the options (src/readtape.c:495-545)."""
    mode: int = tbin.MODE_PE
    ntrks_specified: int = 0
    ntrks: int = 0                     # what an -order= implied
    order: str = ""
    order_is_ww: bool = False
    bpi: float = 0.0
    ips: float = 0.0
    bpi_specified: float = -1.0
    ips_specified: float = -1.0
    find_zeros: bool = False
    differentiate: bool = False
    skip: int = 0
    blklimit: int | None = None
    subsample: int = 1
    verbose: bool = False
    verbose_level: int = 0
    quiet: bool = False
    tap_format: bool = False
    tap_read: bool = False
    even_parity: bool = False
    revparity: int = 0
    invert: bool = False
    fluxdir: str = "neg"
    reverse: bool = False
    deskew: bool = False
    skew: list | None = None
    add_parity: bool = False
    correct: bool = False
    tbin_only: bool = False
    outf: str | None = None
    outp: str = ""
    textfile: bool = False
    num: str | None = None
    char: str | None = None
    linesize: int = 0
    dataspace: int = 0
    linefeed: bool = False
    logging: bool = True
    labels: bool = True
    multiple_tries: bool = True
    filelist: bool = False
    stream: bool = False
    windows: int | None = None         # --windows[=rows]: None not given, 0 the window --stream computes
    peakstats: bool = False
    write: str | None = None           # --write[=host]: "device" / "host"
    tdelta: int | None = None          # --tdelta= ... --gap=: the writer's; None: the format's default
    noise: float | None = None
    jitter: float | None = None
    seed: int | None = None
    gap: int | None = None

    def text_options(self):
        """-textfile's options as the run uses them (src/readtape.c:1940-1946): any number or character type asks for the file; 32 characters a line
        with both a number and a character type, otherwise 64.  None: no text file."""
        from . import textfile as tf
        if not (self.textfile or self.num or self.char):
            return None
        linesize = self.linesize or (32 if (self.num and self.char) else 64)
        return tf.TextOptions(num=self.num, char=self.char, linesize=linesize, dataspace=self.dataspace, linefeed=self.linefeed)

    def resolved_ips(self, header_ips=0.0):
        """src/readtape.c:1341-1343, 1649-1650: -ips= wins over the header, the header over -gcr's 25, and 50 is the default"""
        return self.ips_specified if self.ips_specified >= 0 else (header_ips or self.ips or 50.0)

    def resolved_bpi(self, mode, header_bpi=0.0):
        """src/readtape.c:1338-1340, 1651-1654: -bpi= wins over the header, the header over -whirlwind's 100; GCR is 9042 whatever was said; 0: detect it"""
        if mode == tbin.MODE_GCR:
            return 9042.0
        return self.bpi_specified if self.bpi_specified >= 0 else (header_bpi or self.bpi)


def _key(arg, keyword):
    return arg.upper() == keyword


def _value(arg, keyword):
    """the text behind "KEYWORD", or None if the argument does not begin with it"""
    return arg[len(keyword):] if arg[:len(keyword)].upper() == keyword else None


def parse_int(text):
    """An option's integer (opt_int, src/readtape.c:822-843): decimal, 0x hex, 0b binary, or octal behind a leading 0.  None: not a number."""
    if text[:1] == "0":
        rest = text[1:]
        if rest[:1] in ("x", "X"):
            m = re.fullmatch(r"[0-9a-fA-F]+", rest[1:])
            return int(rest[1:], 16) if m else None
        if rest[:1] in ("b", "B"):
            return int(rest[1:] or "0", 2) if re.fullmatch(r"[01]*", rest[1:]) else None
        if rest == "":
            return 0
        return int(rest, 8) if re.fullmatch(r"[0-7]+", rest) else None
    return int(text) if re.fullmatch(r"[+-]?[0-9]+", text) else None


def _int(arg, keyword, lo, hi):
    """-> (matched, value): matched is False where the keyword is another one, the text no integer, or the value outside lo..hi"""
    text = _value(arg, keyword)
    if text is None:
        return False, 0
    n = parse_int(text)
    if n is None or n < lo or n > hi:
        return False, 0
    return True, n


def _float(arg, keyword, lo, hi):
    text = _value(arg, keyword)
    if text is None or not re.fullmatch(r"[+-]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?", text):
        return False, 0.0
    x = float(np.float32(text))
    return (True, x) if lo <= x <= hi else (False, 0.0)


WW_ROLES = "CLMclm"


def _parse_order(o: Options, text):
    """parse_track_order (src/readtape.c:877-919) -> False for a string that is no track order (the argument is then a bad option)"""
    n = len(text)
    nheads = len(o.order) if o.order else 0
    if nheads and n != nheads:
        raise fatal(f"-order length doesn't match nheads={nheads}")
    if not MINTRKS <= n <= MAXTRKS:
        raise fatal(f"-order can't imply ntrks={n}")
    if o.mode == tbin.MODE_WW:
        used = [ch for ch in text if ch != "x"]
        for ch in used:
            if ch not in WW_ROLES:
                raise fatal(f"bad Whirlwind track order symbol: {ch} in {text}")
            if used.count(ch) > 1:
                raise fatal(f"you already assigned track type {ch}")
        for ch, what in (("C", "clock"), ("M", "MSB"), ("L", "LSB")):
            if ch not in used:
                raise fatal(f"primary {what} track ('{ch}') wasn't assigned")
        o.order, o.order_is_ww, o.ntrks = text, True, len(used)
        return True
    done = 0
    for ch in text:
        if ch in "pP":
            t = n - 1
        elif ch.isdigit() and ch.isascii() and int(ch) <= n - 2:
            t = int(ch)
        else:
            return False
        done |= 1 << t
    if done + 1 != 1 << n:                                    # (a permutation of 0 .. ntrks-1)
        return False
    o.order, o.order_is_ww = text, False
    if o.ntrks == 0:
        o.ntrks = n
    return True


def _parse_skew(o: Options, text):
    """parse_skew (src/readtape.c:921-934): exactly -ntrks= integers, commas between them"""
    if o.ntrks_specified <= 0:
        raise fatal("must specify ntrks= to use skew=")
    vals, rest = [], text
    for t in range(o.ntrks_specified):
        m = re.match(r"\s*[+-]?[0-9]+", rest)
        if not m:
            raise fatal(f"bad skew at: {rest}")
        vals.append(int(m.group()))
        rest = rest[m.end():].lstrip(" ")
        if t < o.ntrks_specified - 1:
            if rest[:1] != ",":
                raise fatal(f"missing comma in skew list at: {rest[1:]}")
            rest = rest[1:].lstrip(" ")
    if rest:
        raise fatal(f"extra crap in skew list: {rest}")
    o.skew, o.deskew = vals, True


NUMS = {"HEX": "hex", "OCTAL": "octal"}
CHARS = {"ASCII": "ascii", "EBCDIC": "ebcdic", "BCD": "bcd", "B5500": "b5500", "SIXBIT": "sixbit", "SDSM": "sdsm", "SDS": "sds", "ADAGE": "adage",
         "ADAGETAPE": "adagetape", "FLEXO": "flexo", "CDC": "cdc", "UNIVAC": "univac"}
FLAGS = {"ZEROS": ("find_zeros", True), "DIFFERENTIATE": ("differentiate", True), "TAP": ("tap_format", True), "TAPREAD": ("tap_read", True),
         "EVEN": ("even_parity", True), "INVERT": ("invert", True), "REVERSE": ("reverse", True), "DESKEW": ("deskew", True),
         "ADDPARITY": ("add_parity", True), "CORRECT": ("correct", True), "NOCORRECT": ("correct", False), "TBIN": ("tbin_only", True),
         "TEXTFILE": ("textfile", True), "LINEFEED": ("linefeed", True), "NOLOG": ("logging", False), "NOLABELS": ("labels", False),
         "NM": ("multiple_tries", False), "NRZI": ("mode", tbin.MODE_NRZI), "PE": ("mode", tbin.MODE_PE),
         "FLUXDIR=POS": ("fluxdir", "pos"), "FLUXDIR=NEG": ("fluxdir", "neg"), "FLUXDIR=AUTO": ("fluxdir", "auto")}
INTS = {"SKIP=": ("skip", 0, INT_MAX), "BLKLIMIT=": ("blklimit", 0, INT_MAX), "SUBSAMPLE=": ("subsample", 1, INT_MAX),
        "REVPARITY=": ("revparity", 0, INT_MAX), "LINESIZE=": ("linesize", 4, MAXLINE), "DATASPACE=": ("dataspace", 0, MAXLINE)}


def not_built(option, why):
    return CliExit(2, f"{option}: {why}\n")


def parse_option(o: Options, option: str) -> bool:
    """One argument (parse_option, src/readtape.c:936-1022).  False: it does not begin with '-', the options are over.  A bad option, or one whose value is
    out of range, raises CliExit(99); an option of the reference that is not built here raises CliExit(2)."""
    if not option.startswith("-"):
        return False
    arg = option[1:]
    up = arg.upper()
    if up == "-STREAM":                                       # (ours, not the reference's: the long options)
        o.stream = True
        return True
    if up == "-PEAKSTATS":
        o.peakstats = True
        return True
    if up == "-WINDOWS":
        o.windows = 0
        return True
    if up in ("-WRITE", "-WRITE=HOST"):
        o.write = "host" if up.endswith("HOST") else "device"
        return True
    for kw, name, lo, hi in (("-TDELTA=", "tdelta", 1, 10_000_000), ("-SEED=", "seed", 0, INT_MAX), ("-GAP=", "gap", 0, INT_MAX)):
        ok, n = _int(arg, kw, lo, hi)
        if ok:
            setattr(o, name, n)
            return True
    for kw, name, hi in (("-NOISE=", "noise", 1e6), ("-JITTER=", "jitter", 1.0)):
        ok, x = _float(arg, kw, 0.0, hi)
        if ok:
            setattr(o, name, x)
            return True
    ok, n = _int(arg, "-WINDOWS=", 1024, 1 << 30)
    if ok:
        o.windows = -(-n // 1024) * 1024                      # (windows are cut on the 1024-row grid)
        return True
    ok, n = _int(arg, "NTRKS=", MINTRKS, MAXTRKS)
    if ok:
        o.ntrks_specified = n
        return True
    text = _value(arg, "ORDER=")
    if text is not None and _parse_order(o, text):
        return True
    if up == "GCR":
        o.mode, o.ips = tbin.MODE_GCR, 25.0
        return True
    if up == "WHIRLWIND":
        o.mode, o.bpi, o.multiple_tries = tbin.MODE_WW, 100.0, False
        return True
    for kw, name in (("BPI=", "bpi_specified"), ("IPS=", "ips_specified")):
        ok, x = _float(arg, kw, *((100, 10000) if kw == "BPI=" else (10, 200)))
        if ok:
            setattr(o, name, x)
            return True
    for kw, (name, lo, hi) in INTS.items():
        ok, n = _int(arg, kw, lo, hi)
        if ok:
            setattr(o, name, n)
            return True
    if _int(arg, "SHOWIBG=", 0, INT_MAX)[0]:
        raise not_built(option, "the report on interblock gaps is not built")
    ok, n = _int(arg, "V", 0, 255)
    if ok:
        o.verbose, o.verbose_level = True, n
        return True
    if _int(arg, "D", 0, 255)[0] or up == "D":
        raise not_built(option, "the reference's debugging output is not built")
    if up in FLAGS:
        name, value = FLAGS[up]
        setattr(o, name, value)
        return True
    if up == "ADJSKEW":
        raise not_built(option, "the running adjustment of the head skew is not built")
    text = _value(arg, "SKEW=")
    if text is not None:
        _parse_skew(o, text)
        return True
    text = _value(arg, "OUTF=")
    if text is not None:
        o.outf = text
        return True
    text = _value(arg, "OUTP=")
    if text is not None:
        o.outp = text
        return True
    for kw, what in (("SUMT=", "text"), ("SUMC=", "CSV")):
        if _value(arg, kw) is not None:
            raise not_built(option, f"the {what} summary file is not built")
    if up == "OCTAL2":
        o.num, o.dataspace = "octal2", 2
        return True
    if up in NUMS:
        o.num = NUMS[up]
        return True
    if up in CHARS:
        o.char = CHARS[up]
        return True
    if len(arg) == 1:                                         # single-character switches
        if up in ("H", "?"):
            raise CliExit(1, "", usage=True)
        if up == "M":
            o.multiple_tries = True
        elif up == "L":
            o.logging = True
        elif up == "V":
            o.verbose, o.verbose_level, o.quiet = True, 1, False
        elif up == "Q":
            o.quiet, o.verbose = True, False
        elif up == "F":
            o.filelist = True
        else:
            raise CliExit(99, f"bad option: {option}\n")
        return True
    raise CliExit(99, f"bad option: {option}\n")


def parse_args(argv):
    """-> (Options, the arguments from the first one that is no option on)"""
    o = Options()
    for i, a in enumerate(argv):
        if not parse_option(o, a):
            return o, list(argv[i:])
    return o, []


# ---- the input and its parameter sets ----
def split_ext(name):
    """-> (name without a .tap / .csv / .tbin extension of any letter case, that extension or "")  (src/readtape.c:1955-1965)"""
    dot = name.rfind(".")
    if dot >= 0 and name[dot:].lower() in (".tap", ".csv", ".tbin"):
        return name[:dot], name[dot:]
    return name, ""


def find_parms(base, mode, cwd=None):
    """The parameter-set file of a run, or None: <base>.parms, then <MODE>.parms beside the base name, then <MODE>.parms in the current directory."""
    name = MODE_NAMES[mode] + ".parms"
    tries = [base + ".parms"]
    if os.path.dirname(base):
        tries.append(os.path.join(os.path.dirname(base), name))
    tries.append(os.path.join(cwd or os.getcwd(), name))
    return next((p for p in tries if os.path.isfile(p)), None)


def parms_options(text):
    """The options on the `readtape` lines of a .parms text (src/parmsets.c:253-258), in order."""
    found = []
    for line in text.splitlines():
        s = line.lstrip(" \t")
        if s[:8].lower() == "readtape":
            found += s[8:].split()
    return found


def find_input(base, ext, tbin_only):
    """-> (path, "csv" | "tbin")  (src/readtape.c:1586-1596)"""
    if not tbin_only and ext.lower() != ".tbin" and os.path.isfile(base + ".csv"):
        return base + ".csv", "csv"
    if os.path.isfile(base + ".tbin"):
        return base + ".tbin", "tbin"
    raise fatal(f"Unable to open input file \"{base}\" .tbin or .csv")


def read_tbin_payload(path, skip):
    """-> (header, rows): the payload up to the first end marker BEHIND the skipped rows (the reference does not look at those, src/readtape.c:1634-1641)"""
    try:
        hdr, off = tbin.read_header(path)
        payload = np.fromfile(path, dtype="<i2", offset=off)
    except (OSError, ValueError) as e:
        raise fatal(str(e))
    nfull = payload.size // hdr.ntrks
    rows = payload[: nfull * hdr.ntrks].reshape(nfull, hdr.ntrks)
    ends = np.flatnonzero(rows[skip:, 0] == tbin.END_MARK)
    if ends.size:
        rows = rows[: skip + int(ends[0])]
    return hdr, rows


def csv_columns(path):
    """the commas of the second title line (src/readtape.c:1610-1616)"""
    try:
        with open(path, "rb") as f:
            f.readline()
            second = f.readline()
    except OSError as e:
        raise fatal(str(e))
    if not second:
        raise fatal("Can't read second CSV title line")
    return second.count(b",")


# ---- one run ----
def _say(out, o, text):
    if not o.quiet:
        out.write(text)


def _decode_options(o: Options):
    from . import pipeline
    return pipeline.DecodeOptions(multiple_tries=o.multiple_tries, correct=o.correct, even_parity=o.even_parity, revparity=o.revparity,
                                  add_parity=o.add_parity, verbose=o.verbose)


def _stream_refusal(o: Options, mode):
    if not o.tap_format:
        return "--stream writes one SIMH file: give -tap"
    if mode == tbin.MODE_WW:
        return "--stream is not for Whirlwind tapes (one chain, no independent windows)"
    if o.text_options() is not None:
        return "--stream writes no text file: leave -textfile and its options out"
    if o.blklimit is not None:
        return "--stream has no -blklimit"
    if o.labels:
        return "--stream does not decode tape labels: give -nolabels"
    if o.order or o.bpi_specified >= 0 or o.ips_specified >= 0 or o.ntrks_specified:
        return "--stream takes the tracks, their order, the density and the speed from the .tbin header"
    return None


def _stream_window(o: Options, path):
    """the window --stream and --windows take by default (a short file: no buffers for windows it does not have) -> (window rows, halo rows)"""
    from . import ingest
    used = max(0, ingest._payload_geometry(path)[2] - o.skip) // o.subsample
    window = min(1 << 24, max(1024, -(-used // 1024) * 1024))
    return window, min(1 << 17, window)


def _decode_windows(o: Options, path, hdr, mode, out_base, log_path, parms_text, text_opts):
    """--windows: the file through ingest.decode_file_windows with the options as the resident path takes them -> its statistics"""
    from . import ingest
    window, halo = _stream_window(o, path)
    if o.windows:
        window, halo = o.windows, min(1 << 17, o.windows)
    cfgkw = {k: v for k, v in (("invert", o.invert), ("find_zeros", o.find_zeros), ("differentiate", o.differentiate)) if v}
    return ingest.decode_file_windows(path, out_base=out_base, log_path=log_path, tap_format=o.tap_format, labels=o.labels, blklimit=o.blklimit, textfile=text_opts,
                                      peakstats=o.peakstats, quiet=o.quiet, hdr_overrides=dict(order=o.order or None, bpi=hdr.bpi, ips=hdr.ips, mode=mode),
                                      in_name=path, parms_text=parms_text, window_rows=window, halo_rows=halo, opts=_decode_options(o), cfgkw=cfgkw or None,
                                      subsample=o.subsample, skip=o.skip, deskew=o.deskew and o.skew is None, skew=o.skew)


def decode_file(o: Options, name, fe_factory, out, outbase_of):
    """One tape: §3-§4 of the module's grammar.  -> True if every block was clean ("ok")."""
    from . import csvin, pipeline
    base, ext = split_ext(name)
    out_base = outbase_of(base)
    path, kind = find_input(base, ext, o.tbin_only)
    _say(out, o, f"\nreading file \"{path}\"\nthe output files will be \"{out_base}.xxx\"\n")
    hdr = rows = None
    if kind == "tbin":
        if o.stream or o.windows is not None:
            try:
                hdr, _ = tbin.read_header(path)
            except (OSError, ValueError) as e:
                raise fatal(str(e))
        else:
            hdr, rows = read_tbin_payload(path, o.skip)
    mode = hdr.mode if (hdr is not None and hdr.mode != 0) else o.mode      # a header that knows its mode wins (src/readtape.c:1335-1337)
    if mode not in MODE_NAMES:
        raise fatal("bad mode in read_parms")
    # the parameter sets, and the options that come with them (src/parmsets.c:337-377, 253-258)
    parms_path = find_parms(base, mode)
    parms_text = None
    if parms_path:
        with open(parms_path) as f:
            parms_text = f.read()
        _say(out, o, f"\nreading parmsets from file {parms_path}\n")
        for extra in parms_options(parms_text):
            if not parse_option(o, extra):
                raise fatal(f"bad option from parms file: {extra}")
        if hdr is None or hdr.mode == 0:
            mode = o.mode
    if mode == tbin.MODE_WW and o.multiple_tries:
        raise fatal("Sorry, multiple decoding tries is not implemented yet for Whirlwind")
    text_opts = o.text_options()
    if o.windows is not None:
        why = ("--stream and --windows are two decodes: give one" if o.stream else "--windows reads a .tbin file" if kind != "tbin" else
               "--windows is not for Whirlwind tapes (one chain, no independent windows)" if mode == tbin.MODE_WW else None)
        if why:
            raise CliExit(2, why + "\n")
    if o.stream:
        why = "--stream reads a .tbin file" if kind != "tbin" else _stream_refusal(o, mode)
        if o.peakstats:
            why = "--stream gathers no flux-transition statistics: leave --peakstats out (its bins are fixed by the tape's first transition, which only the first window sees)"
        if why:
            raise CliExit(2, why + "\n")
    if kind == "csv":
        ntrks = o.ntrks_specified or o.ntrks or csv_columns(path)
        conv = dict(ntrks=ntrks, mode=mode, bpi=o.resolved_bpi(mode), ips=o.resolved_ips())
        try:
            if fe_factory is None:
                hdr, rows, _ = csvin.read_csv_device(path, **conv)
            else:
                hdr, rows, _ = csvin.read_csv(path, **conv)
        except (OSError, ValueError) as e:
            raise fatal(str(e))
    else:
        if o.ntrks_specified and o.ntrks_specified != hdr.ntrks:
            _say(out, o, f"*** WARNING *** .tbin file says {hdr.ntrks} trks but ntrks={o.ntrks_specified}\n")
        if o.order and hdr.trkorder and hdr.trkorder != o.order:
            _say(out, o, f"  the .tbin head order {hdr.trkorder} is being ignored because it was specified as {o.order} on the command line\n")
        hdr = dataclasses.replace(hdr, mode=mode, bpi=o.resolved_bpi(mode, hdr.bpi), ips=o.resolved_ips(hdr.ips))
    if o.skew is not None and len(o.skew) != hdr.ntrks:
        raise fatal(f"ntrks={o.ntrks_specified} doesn't match what we already deduced: {hdr.ntrks}")
    if o.add_parity and hdr.ntrks >= 9:
        raise fatal(f"-parity not allowed with ntrks={hdr.ntrks}")
    if o.stream:
        from . import ingest
        _say(out, o, "the streamed decode writes no log\n")
        cfgkw = {k: v for k, v in (("invert", o.invert), ("find_zeros", o.find_zeros), ("differentiate", o.differentiate)) if v}
        window, halo = _stream_window(o, path)
        try:
            st = ingest.decode_file_streaming(path, out_base + ".tap", window_rows=window, halo_rows=halo, opts=_decode_options(o), cfgkw=cfgkw or None,
                                              subsample=o.subsample, skip=o.skip, deskew=o.deskew and o.skew is None, skew=o.skew)
        except NotImplementedError as e:
            raise CliExit(2, f"{e}\n")
        except (pipeline.ReferenceFatal, ValueError, RuntimeError) as e:
            raise fatal(str(e))
        return bool(st["all_ok"])
    log_path, scratch = (out_base + ".log", None) if o.logging else (None, None)
    if log_path is None and not o.quiet:                      # -nolog: the text goes to the console only
        fd, scratch = tempfile.mkstemp(suffix=".log")
        os.close(fd)
        log_path = scratch
    try:
        try:
            if o.windows is not None:
                stats = _decode_windows(o, path, hdr, mode, out_base, log_path, parms_text, text_opts)
            else:
                stats, _ = pipeline.decode_tape(hdr, rows, None, log_path=log_path, opts=_decode_options(o), fe_factory=fe_factory, skew=o.skew, invert=o.invert,
                                                parms_text=parms_text, find_zeros=o.find_zeros, differentiate=o.differentiate, subsample=o.subsample,
                                                deskew=o.deskew, trkorder=o.order or None, out_base=out_base, in_name=path, tap_format=o.tap_format,
                                                fluxdir=o.fluxdir, reverse=o.reverse, textfile=text_opts, labels=o.labels, blklimit=o.blklimit, skip=o.skip,
                                                peakstats=o.peakstats, quiet=o.quiet)
        finally:
            if log_path and not o.quiet and os.path.exists(log_path):
                with open(log_path, errors="replace") as f:
                    out.write(f.read())
    except NotImplementedError as e:                          # (density detection for PE: the reference's own pre-pass degenerates there)
        raise CliExit(2, f"{e}\n")
    except (pipeline.ReferenceFatal, ValueError, RuntimeError) as e:
        # a fatal assert of the reference's detector, a density that is no standard one, tracks without transitions under -deskew; a .parms text, an order
        # string or a text option the libraries refuse: the reference exits with 99 on each
        raise fatal(str(e))
    finally:
        if scratch and os.path.exists(scratch):
            os.remove(scratch)
    return bool(stats["all_ok"])


def tapread(o: Options, base, ext, out_base, fe_factory, out):
    """-tapread (src/readtape.c:1978-1984, src/tapread.c:53-61): the interpreted text of a SIMH .tap file"""
    from . import textfile as tf
    path = base + ext
    if not os.path.isfile(path) and not ext:
        path = base + ".tap"
    if not os.path.isfile(path):
        raise fatal(f"Unable to open SIMH TAP file \"{path}\"")
    _say(out, o, f"processing {path}\n")
    opts = o.text_options() or tf.TextOptions(linesize=o.linesize or 64, dataspace=o.dataspace, linefeed=o.linefeed)
    ntrks = o.ntrks_specified or 9
    try:
        if fe_factory is None and os.path.getsize(path) >= DEVICE_TEXT_BYTES:
            r = tf.write_text_device(path, out_base, opts, ntrks=ntrks)
        else:
            r = tf.write_text(path, out_base, opts, ntrks=ntrks)
    except tf.TapFormatError as e:
        raise fatal(str(e))
    except ValueError as e:
        raise fatal(str(e))
    _say(out, o, f"created {r['name']}\n")


def write_tape(o: Options, argv, base, ext, out_base, device, out):
    """--write: <base>[.tap] -> <out_base>.tbin (tapewrite.write_tbin / write_tbin_device).  A combination the writer does not take ends with status 2."""
    from . import tapewrite as tw, textfile as tf
    given = [a.upper() for a in argv if a.upper() in ("-NRZI", "-PE", "-GCR", "-WHIRLWIND")]
    why = ("--write does not write Whirlwind tapes: a Whirlwind pulse is two transitions 0.35 cell apart, off the writer's half-cell grid" if "-WHIRLWIND" in given else
           "--write wants the tape's format: -nrzi, -pe or -gcr" if not given else
           "--write renders a .tap image: leave --stream, --windows, -tapread and -f out" if (o.stream or o.windows is not None or o.tap_read or o.filelist) else
           f"--write reads a SIMH .tap file, not {ext}" if ext.lower() not in ("", ".tap") else None)
    if why:
        raise CliExit(2, why + "\n")
    kw = {k: v for k, v in (("tdelta_ns", o.tdelta), ("noise_mv", o.noise), ("jitter", o.jitter), ("gap_samples", o.gap)) if v is not None}
    seed = 1 if o.seed is None else o.seed
    spec = (tw.nrzi_spec(seed=seed, ntrks=o.ntrks_specified or 9, even=o.even_parity, **kw) if o.mode == tbin.MODE_NRZI else
            (tw.pe_spec if o.mode == tbin.MODE_PE else tw.gcr_spec)(seed=seed, ntrks=o.ntrks_specified or 9, even=o.even_parity, **kw))
    if o.bpi_specified >= 0:
        spec.bpi = o.bpi_specified
    if o.ips_specified >= 0:
        spec.ips = o.ips_specified
    path = base + (ext or ".tap")
    if not os.path.isfile(path):
        raise fatal(f"Unable to open SIMH TAP file \"{path}\"")
    _say(out, o, f"rendering {path}\n")
    try:
        if o.write == "host":
            r = tw.write_tbin(path, out_base + ".tbin", spec)
        else:
            r = tw.write_tbin_device(path, out_base + ".tbin", spec, **({} if device is None else dict(_lib_path=device[0], _backend=device[1])))
    except tw.TapeWriteError as e:
        raise CliExit(2, f"--write: {e}\n")
    except tf.TapFormatError as e:
        raise fatal(str(e))
    _say(out, o, f"created {out_base}.tbin: {r['rows']} samples, {r['blocks']} blocks\n")


def run(argv, fe_factory, out, device=None):
    if not argv:
        raise CliExit(4, "", usage=True)
    o, rest = parse_args(argv)
    if not rest:
        raise CliExit(4, "\n*** No <basefilename> given\n\n", usage=True)
    if len(rest) > 1:
        raise CliExit(4, f"\n*** unknown parameter: {rest[0]}\n\n", usage=True)
    base, ext = split_ext(rest[0])
    if base.lower().endswith(".txt"):
        o.filelist, base = True, base[:-4]

    def outbase_of(b):
        if o.outf is not None:
            return o.outf
        return o.outp + b

    if o.write:
        write_tape(o, argv, base, ext, outbase_of(base), device, out)
        return 0
    if o.tap_read or ext.lower() == ".tap":
        if o.stream:
            raise CliExit(2, "--stream decodes a .tbin file, -tapread reads a .tap\n")
        tapread(o, base, ext, outbase_of(base), fe_factory, out)
        return 0
    if o.mode == tbin.MODE_WW and o.multiple_tries:
        raise fatal("Sorry, multiple decoding tries is not implemented yet for Whirlwind")
    if o.filelist:
        try:
            with open(base + ".txt") as f:
                lines = f.read().splitlines()
        except OSError:
            raise fatal(f"Unable to open file list file \"{base}.txt\"")
        for line in lines:
            name = line.strip()
            while name.startswith("-"):                           # leading options: they stay in force for the files behind this one
                option, _, name = name.partition(" ")
                parse_option(o, option)
                name = name.lstrip()
            if not name:
                continue
            ok = decode_file(o, name, fe_factory, out, outbase_of)
            out.write(f"{name}: {'ok' if ok else 'bad'}\n")
        return 0
    ok = decode_file(o, rest[0], fe_factory, out, outbase_of)
    if o.quiet:
        out.write(f"{base}: {'ok' if ok else 'bad'}\n")
    return 0


def main(argv=None, *, fe_factory=None, out=None, device=None) -> int:
    """Runs one command line; returns the exit status.  fe_factory: pipeline.decode_tape's (the tests pass the emulated front end); out: where the console
    text goes (sys.stdout); device: --write's (front-end library path, backend), for the same tests."""
    argv = list(sys.argv[1:] if argv is None else argv)
    out = out or sys.stdout
    try:
        return run(argv, fe_factory, out, device)
    except CliExit as e:
        if e.message:
            sys.stderr.write(e.message)
        if e.usage:
            sys.stderr.write(USAGE)
        return e.status
    finally:
        if hasattr(out, "flush"):
            out.flush()
