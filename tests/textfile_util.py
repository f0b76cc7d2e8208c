"""What the host, the emulated and the GPU tests of the interpreted text dump (readtape_amd/textfile.py; csrc/host/rt_textfile.c, rt_tapread.c; kernels in
csrc/rtfe_textfile.hip) share: hand-made .tap images, the goldens tests/make_textfile_golden.py made from them with the reference, and the cases the device
formatter is run through - the shapes at which a line, a record, a wave's batch or a window ends.  Everything compares byte for byte."""
import ctypes as C
import glob
import os
import struct

import numpy as np

from readtape_amd import csvin, frontend, textfile
from readtape_amd.textfile import TextOptions

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DATE = "Tue Oct 20 12:00:00 2026\n"
EOM = b"\xff\xff\xff\xff"


# ---- images ----
def rec(data, err=False, pad=None, trailer=None):
    """A record: its marker, the data, the pad (default: one byte behind an odd length), the trailing length."""
    data = bytes(data)
    m = len(data) | (0x80000000 if err else 0)
    pad = (len(data) & 1) if pad is None else pad
    return struct.pack("<I", m) + data + b"\0" * pad + struct.pack("<I", m if trailer is None else trailer)


MARK = b"\0\0\0\0"


def rnd(seed, n, lo=0, hi=256):
    return np.random.RandomState(seed).randint(lo, hi, n).astype(np.uint8).tobytes()


ALL = bytes(range(256))
TEXT = (b"\nFIRST LINE AFTER A LINEFEED AT INDEX 0\nodd\n\ntwo in a row above; now exactly thirty-two bytes..\nthen a long line that has to be cut at the line size "
        b"more than once before it ends\nx\n")


def opts_from_args(args):
    """The reference's command-line options -> (TextOptions, ntrks)."""
    o, ntrks = TextOptions(), 9
    for a in args:
        k = a.lower().lstrip("-")
        if k in ("hex", "octal", "octal2"):
            o.num = k
        elif k in textfile.CHARS:
            o.char = k
        elif k.startswith("linesize="):
            o.linesize = int(k[9:])
        elif k.startswith("dataspace="):
            o.dataspace = int(k[10:])
        elif k == "linefeed":
            o.linefeed = True
        elif k.startswith("ntrks="):
            ntrks = int(k[6:])
        else:
            raise ValueError(a)
    return o, ntrks


def cut_date(txt):
    """The text without its second line, and that line."""
    a = txt.index(b"\n") + 1
    b = txt.index(b"\n", a) + 1
    return txt[:a] + txt[b:], txt[a:b]


def golden_cases():
    """name, .tap image, the reference's options."""
    sizes = [1, 2, 3, 31, 32, 33, 65]
    plain = b"".join(rec(rnd(10 + n, n), err=n in (3, 33)) for n in sizes[:4]) + MARK + b"".join(rec(rnd(10 + n, n)) for n in sizes[4:]) + MARK + MARK + EOM
    yield "hex_ebcdic", plain, ["-hex", "-ebcdic"]
    yield "octal_ascii", plain, ["-octal", "-ascii"]
    yield "octal7_bcd", plain, ["-octal", "-bcd", "-ntrks=7"]
    yield "octal2_flexo", plain, ["-octal2", "-flexo"]
    yield "hex", plain, ["-hex", "-linesize=20", "-dataspace=4"]
    yield "octal", plain, ["-octal", "-dataspace=3"]
    yield "octal2", plain, ["-octal2", "-linesize=7"]
    yield "sizes_only", b"".join(rec(rnd(n, 1 + n * 37 % 1500), err=n % 5 == 0) for n in range(24)) + MARK + rec(b"abc") + EOM, ["-linesize=40"]
    chars = MARK + rec(ALL) + rec(ALL[1:] + ALL[:64]) + EOM                       # every byte value at an even and at an odd index
    nums = ["-hex", None, "-octal", "-octal2"]
    for k, c in enumerate(textfile.CHARS[1:]):
        num = nums[k % 4]
        yield "char_" + c, chars, ([num] if num else []) + ["-" + c] + (["-linesize=48"] if k % 3 == 0 else [])
    odd = rec(rnd(3, 5)) + rec(rnd(4, 6)) + rec(rnd(5, 7)) + rec(rnd(6, 8)) + rec(rnd(7, 15)) + rec(rnd(8, 1)) + EOM
    yield "octal2_odd5", odd, ["-octal2", "-sixbit", "-linesize=5"]
    yield "octal2_odd7_ds1", odd, ["-octal2", "-ascii", "-linesize=7", "-dataspace=1"]
    yield "octal2_odd5_ds3", odd, ["-octal2", "-cdc", "-linesize=5", "-dataspace=3", "-ntrks=7"]
    for ds in (0, 1, 8, 5, 50):                                                  # none, every byte, dividing the line, not dividing it, larger than it
        yield f"hex_ascii_ds{ds}", plain, ["-hex", "-ascii", f"-dataspace={ds}"]
    yield "octal_ds5_7", plain, ["-octal", "-univac", "-dataspace=5", "-ntrks=7", "-linesize=12"]
    lf = rec(TEXT) + rec(b"\n") + rec(b"\n\n") + rec(b"ab\n") + rec(b"a\nb") + MARK + rec(TEXT[1:]) + EOM
    yield "lf_ascii", lf, ["-ascii", "-linefeed", "-linesize=32"]
    yield "lf_hex_ascii", lf, ["-hex", "-ascii", "-linefeed"]
    yield "lf_octal2_flexo", lf, ["-octal2", "-flexo", "-linefeed", "-linesize=16"]
    yield "lf_octal_sds", lf, ["-octal", "-sds", "-linefeed", "-linesize=9", "-dataspace=4"]
    yield "lf_ignored", lf, ["-hex", "-ascii"]
    yield "wide_prefix", rec(bytes(33 + i % 90 for i in range(9999))) + rec(bytes(33 + i % 89 for i in range(10000)), err=True) + EOM, ["-ascii", "-linesize=400"]
    yield "marks", MARK + MARK + rec(b"between") + MARK + EOM, ["-hex", "-ascii"]
    yield "no_end", rec(b"the end marker is missing") + MARK, ["-hex", "-ascii"]
    yield "no_end_partial", rec(b"two stray bytes follow") + b"\xff\xff", ["-ascii"]
    for pad in range(5):
        yield f"pad{pad}", rec(b"abcde", pad=pad) + rec(b"next") + EOM, ["-hex", "-ascii"]
    # what the reference stops on
    yield "fatal_pad5", rec(b"abcde", pad=5) + rec(b"next") + EOM, ["-hex", "-ascii"]
    yield "fatal_gap", rec(b"before") + b"\xfe\xff\xff\xff" + rec(b"after") + EOM, ["-hex", "-ascii"]
    yield "fatal_class", rec(b"before") + struct.pack("<I", 0x01000004) + b"datadata" + EOM, ["-ascii"]
    yield "fatal_zero", rec(b"before") + struct.pack("<I", 0x80000000) + EOM, ["-ascii"]
    yield "fatal_big", rec(b"before") + struct.pack("<I", 131072) + b"x" * 100 + EOM, ["-ascii"]
    yield "fatal_short", rec(b"before") + struct.pack("<I", 50) + b"x" * 20, ["-ascii"]
    yield "fatal_no_trailer", rec(b"before") + struct.pack("<I", 6) + b"sixsix" + b"\xff\xff", ["-ascii"]
    yield "fatal_sizes", rec(b"a") + rec(b"bb") + struct.pack("<I", 0x80000000), []


DECODE_GOLDENS = {"decode_nrzi9": ("case_nrzi9", ["-hex", "-ebcdic"], []), "decode_pe": ("case_pe", ["-octal", "-ascii", "-linesize=16"], []),
                  "decode_ww": ("case_ww", ["-octal2", "-flexo"], []), "decode_nrzi7_parity": ("case_nrzi7", ["-octal", "-bcd"], ["-addparity"])}

GOLDENS = sorted(os.path.basename(p)[len("text_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "text_*.npz")))
EXPECTED_GOLDENS = [c[0] for c in golden_cases()]
TAP_GOLDENS = [n for n in EXPECTED_GOLDENS if not n.startswith("fatal_")]
FATAL_GOLDENS = [n for n in EXPECTED_GOLDENS if n.startswith("fatal_")]


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, f"text_{name}.npz"))
    g = dict(opts=[str(x) for x in z["opts"]], name=str(z["name"]), txt=z["txt"].tobytes(), date=z["date"].tobytes(), status=int(z["status"]))
    for k in ("tap", "tapout"):
        if k in z.files:
            g[k] = z[k].tobytes()
    if "tape" in z.files:
        g["tape"] = str(z["tape"])
        g["ref_opts"] = [str(x) for x in z["ref_opts"]]
    return g


def same(got, want, what=""):
    if got != want:
        n = min(len(got), len(want))
        i = next((k for k in range(n) if got[k] != want[k]), n)
        line = want.count(b"\n", 0, i)
        raise AssertionError(f"{what}: texts differ at byte {i} (line {line}) of {len(got)} / {len(want)}:\n got  {got[max(0, i - 60): i + 60]!r}\n want {want[max(0, i - 60): i + 60]!r}")


def host_text(tmp_path, image, opts, ntrks=9, tag="h"):
    """write_text's file, the date line cut out -> (text, its name behind the base's dot, the exception or None)."""
    os.makedirs(tmp_path / tag, exist_ok=True)
    base = str(tmp_path / tag / "g")
    err = None
    try:
        textfile.write_text(image, base, opts, ntrks=ntrks, created=DATE)
    except textfile.TapFormatError as e:
        err = e
    name = textfile.text_name(base, opts)
    body, date = cut_date(open(name, "rb").read())
    assert date.endswith(b" on " + DATE.encode()), date
    return body.replace(base.encode(), b"g"), os.path.basename(name)[2:], err


# ---- the device path ----
def device_text(tmp_path, be, lib_path, image, opts, ntrks=9, tag="d", **kw):
    """write_text_device's file, the date line cut out -> (text, info or None, the exception or None)."""
    os.makedirs(tmp_path / tag, exist_ok=True)
    base = str(tmp_path / tag / "g")
    info = err = None
    try:
        info = textfile.write_text_device(image, base, opts, ntrks=ntrks, created=DATE, _lib_path=lib_path, _backend=be, **kw)
    except textfile.TapFormatError as e:
        err = e
    body, date = cut_date(open(textfile.text_name(base, opts), "rb").read())
    return body.replace(base.encode(), b"g"), info, err


def body_of(text):
    """What stands between the title and the trailer."""
    a = text.index(b"\n\n") + 2
    return text[a: text.rindex(b"end of file\n\n")]


def run_golden(name, tmp_path, be, lib_path=None):
    """The device's file is the reference's - or, for the list of block sizes, the device refuses."""
    g = load_golden(name)
    opts, ntrks = opts_from_args(g["opts"])
    if opts.num is None and opts.char is None:
        try:
            device_text(tmp_path, be, lib_path, g["tap"], opts, ntrks)
        except ValueError as e:
            assert "block sizes" in str(e)
            return
        raise AssertionError("the list of block sizes was not refused")
    got, info, err = device_text(tmp_path, be, lib_path, g["tap"], opts, ntrks)
    assert (err is None) == (g["status"] == 0), err
    same(got, g["txt"], name)


def run_same_as_host(tmp_path, be, lib_path, image, opts, ntrks=9, what="", **kw):
    want, _, herr = host_text(tmp_path, image, opts, ntrks)
    got, info, derr = device_text(tmp_path, be, lib_path, image, opts, ntrks, **kw)
    assert (herr is None) == (derr is None)
    same(got, want, what or repr(opts))
    return info


def lengths_image(ls, seed=1):
    """Records of 1, 2, 3, ls - 1, ls, ls + 1 and 2 ls + 1 bytes, a mark between them, the third and the last flagged."""
    out = b""
    for k, n in enumerate((1, 2, 3, ls - 1, ls, ls + 1, 2 * ls + 1)):
        out += rec(rnd(seed + k, n), err=k in (2, 6)) + (MARK if k == 3 else b"")
    return out + EOM


# (number type, character type, linesize, dataspace, ntrks): every number type alone and with a character type, every character type alone once, octal at 7
# and 9 tracks, octal2 at odd line sizes, -dataspace none / every byte / dividing the line / not dividing it / larger than it
OPTION_SHAPES = [("hex", None, 0, None, 9), ("octal", None, 0, None, 9), ("octal", None, 16, 4, 7), ("octal2", None, 0, None, 9), ("octal2", None, 0, 0, 7),
                 (None, "ascii", 0, None, 9), (None, "flexo", 20, None, 9), ("hex", "ebcdic", 0, None, 9), ("octal", "bcd", 0, None, 7), ("octal", "sixbit", 12, 5, 9),
                 ("octal2", "flexo", 0, None, 9), ("octal2", "ascii", 5, None, 9), ("octal2", "adage", 7, 1, 9), ("octal2", "cdc", 399, 3, 7), ("octal2", "sds", 7, 7, 9),
                 ("hex", "ascii", 32, 0, 9), ("hex", "ascii", 32, 1, 9), ("hex", "ascii", 32, 8, 9), ("hex", "ascii", 32, 5, 9), ("hex", "ascii", 32, 50, 9),
                 ("hex", "univac", 400, 400, 9), ("octal", "b5500", 4, 3, 9), ("hex", "adagetape", 33, 2, 9), (None, "sdsm", 4, None, 9)]


def shape_opts(shape):
    num, char, ls, ds, ntrks = shape
    return TextOptions(num, char, ls, ds), ntrks


def run_option_shape(shape, tmp_path, be, lib_path=None):
    opts, ntrks = shape_opts(shape)
    ls = shape[2] or (32 if shape[0] and shape[1] else 64)
    run_same_as_host(tmp_path, be, lib_path, lengths_image(ls, seed=ls), opts, ntrks, what=repr(shape))


def run_wide_prefix(tmp_path, be, lib_path=None):
    """The length prefix widens at 10000 bytes, and again at 100000; the longest record there is."""
    img = rec(rnd(1, 9999)) + rec(rnd(2, 10000), err=True) + MARK + rec(rnd(3, 131071)) + rec(rnd(4, 100000)) + EOM
    run_same_as_host(tmp_path, be, lib_path, img, TextOptions("hex", "ebcdic", 400), what="wide prefix")
    run_same_as_host(tmp_path, be, lib_path, img, TextOptions("octal2", None, 399), what="wide prefix, octal2")


LINEFEED_SHAPES = [(None, "ascii", 32, None, 9), ("hex", "ascii", 16, None, 9), ("octal2", "flexo", 16, None, 9), ("octal2", "flexo", 5, None, 9), ("octal", "ascii", 9, 4, 7),
                   ("octal2", None, 6, 0, 9), (None, "flexo", 20, None, 9), ("hex", "flexo", 16, None, 9)]


def linefeed_image():
    """A 0x0a at index 0, at odd and even indices, two in a row, exactly on a linesize boundary (16 and 32), as the last byte; stretches longer than a line;
    and - for the Flexowriter code's high / low halves - breaks that leave a line starting at an odd index."""
    body = bytearray(rnd(9, 300, 32, 127))
    for i in (0, 5, 6, 16, 17, 32, 64, 99, 100, 101, 160, 299):
        body[i] = 10
    return (rec(bytes(body)) + rec(TEXT) + rec(b"\n") + rec(b"\n\n\n") + MARK + rec(b"a\n") + rec(b"ab\n") + rec(b"\nab", err=True) + rec(rnd(3, 70) + b"\n" + rnd(4, 69)) + EOM)


def run_linefeed_shape(shape, tmp_path, be, lib_path=None):
    opts, ntrks = shape_opts(shape)
    opts.linefeed = True
    run_same_as_host(tmp_path, be, lib_path, linefeed_image(), opts, ntrks, what=repr(shape))
    run_same_as_host(tmp_path, be, lib_path, linefeed_image(), opts, ntrks, what=repr(shape) + " in windows", window_bytes=64)


def run_kernel_cuts(tmp_path, be, lib_path=None):
    """Lines across the kernel's own cuts: a record of r bytes in front moves every later line by a byte, so that over r = 1 .. 17 a batch's last line ends in
    front of, on and behind a 16-byte boundary of the text; records of more lines than a batch; and windows that end behind every record."""
    for opts in (TextOptions(None, "ascii", 5), TextOptions("hex", "ascii", 8)):
        for r in range(1, 18):
            img = rec(rnd(r, r, 33, 127)) + rec(rnd(40 + r, 5 * 64 + 3, 33, 127)) + MARK + rec(rnd(80 + r, 5 * 130, 33, 127), err=True) + EOM
            info = run_same_as_host(tmp_path, be, lib_path, img, opts, what=f"shift {r}")
            assert info["windows"] == 1 and info["lines"] == 1 + sum(-(-n // opts.linesize) for n in (r, 5 * 64 + 3, 5 * 130))
    img = b"".join(rec(rnd(k, 1 + k % 40)) + (MARK if k % 7 == 0 else b"") for k in range(60)) + EOM
    info = run_same_as_host(tmp_path, be, lib_path, img, TextOptions("hex", "ebcdic"), what="a window a record", window_bytes=1)
    assert info["windows"] == 60 + 9
    info = run_same_as_host(tmp_path, be, lib_path, img, TextOptions("hex", "ebcdic"), what="windows of a few records", window_bytes=200)
    assert 5 < info["windows"] < 30


def run_empty_and_missing_end(tmp_path, be, lib_path=None):
    for img in (EOM, b"", MARK, rec(b"x"), MARK + MARK + rec(b"xy") + MARK):
        run_same_as_host(tmp_path, be, lib_path, img, TextOptions("hex", "ascii"), what=repr(img))


class Format:
    """rtfe_text_format alone on a backend's memory, 64 canary bytes behind text_cap."""

    def __init__(self, be, lib_path=None):
        self.be, self.lib, self.dev = be, frontend._load_library(lib_path), csvin._Dev(be, False)

    def dopts(self, opts, ntrks=9, verbose=0):
        o = textfile.c_options(opts, ntrks)
        return (C.c_int * 7)(o.numtype, o.chartype, o.linesize, o.dataspace, o.linefeed, o.ntrks, verbose)

    def __call__(self, image, opts, ntrks=9, cap=None, nlf=None, verbose=0, items=None):
        be, lib, dev = self.be, self.lib, self.dev
        img = np.frombuffer(image, np.uint8)
        if items is None:
            items = np.ascontiguousarray(textfile.read_tap(image))
        d = self.dopts(opts, ntrks, verbose)
        n = len(items)
        nlf = image.count(b"\n") if nlf is None else nlf
        ip = items.ctypes.data if n else None
        full = int(lib.rtfe_text_format_max_bytes(ip, n, nlf, d))
        cap = full if cap is None else cap
        canary = bytes([0xA5]) * 64
        d_text = dev.alloc(cap + 64)
        be.upload(d_text, b"\0" * cap + canary)
        d_img, d_items, out = dev.alloc(max(img.size, 1)), dev.alloc(max(items.nbytes, 1)), dev.alloc(32)
        if img.size:
            be.upload(d_img, image)
        if n:
            be.upload(d_items, items.tobytes())
        sb = max(int(lib.rtfe_text_format_scratch_bytes(ip, n, nlf, d)), 16)
        scratch = dev.alloc(sb)
        rc = lib.rtfe_text_format(be.ptr(d_img), img.size, ip, be.ptr(d_items), n, nlf, d, be.ptr(d_text), cap, be.ptr(scratch), sb, be.ptr(out), be.stream())
        if rc != 0:
            return rc, lib.rtfe_last_error().decode(), None
        be.sync()
        o = textfile._Out.from_buffer_copy(bytes(be.to_numpy(out[:32], np.uint8)))
        got = bytes(be.to_numpy(d_text[: cap + 64], np.uint8))
        assert got[cap:] == canary, "rtfe_text_format wrote behind text_cap"
        return 0, o, got[:cap]


def run_bounds(tmp_path, fmt):
    """A text buffer one byte too small (and much too small, and empty): the flag is set, the length is right, the bytes that fit are written and the guard
    behind the buffer is untouched.  A linefeed count that is too small: RTFE_TEXT_SCRATCH_FULL, and no text at all."""
    for opts, img in ((TextOptions("hex", "ebcdic"), lengths_image(32) [:-4] + rec(rnd(5, 3000)) + EOM), (TextOptions(None, "ascii", 16, linefeed=True), linefeed_image()),
                      (TextOptions("octal", "bcd"), lengths_image(32))):
        ntrks = 7 if opts.num == "octal" else 9
        body = body_of(host_text(tmp_path, img, opts, ntrks)[0])
        rc, o, got = fmt(img, opts, ntrks)
        assert rc == 0 and o.flags == 0 and o.bytes == len(body), (rc, o.flags, o.bytes, len(body))
        same(got[: o.bytes], body, "the whole body")
        assert o.lines == body.count(b"\n")
        for cap in (len(body) - 1, len(body) - 17, 100, 16, 0):
            rc, o, got = fmt(img, opts, ntrks, cap=cap)
            assert rc == 0 and o.flags == textfile.TEXT_FULL and o.bytes == len(body), (cap, o.flags, o.bytes)
            same(got, body[:cap], f"cap {cap}")
        rc, o, got = fmt(img, opts, ntrks, cap=len(body))
        assert rc == 0 and o.flags == 0
        same(got, body, "a buffer that just fits")
    img = linefeed_image()
    full = fmt(img, TextOptions(None, "ascii", 16, linefeed=True))[1]
    rc, o, got = fmt(img, TextOptions(None, "ascii", 16, linefeed=True), cap=4096, nlf=3)
    assert rc == 0 and o.flags & textfile.TEXT_SCRATCH_FULL and o.stretches == full.stretches and got == b"\0" * 4096, o.flags


def run_refusals(fmt):
    img = rec(b"abc") + EOM
    d = fmt.dopts(TextOptions())
    assert fmt.lib.rtfe_text_format_max_bytes(None, 0, 0, d) == 0 and "block sizes" in fmt.lib.rtfe_last_error().decode()
    rc, msg, _ = fmt(img, TextOptions("hex"), verbose=1)
    assert rc == -51 and "verbose" in msg
    rc, msg, _ = fmt(img, TextOptions(), items=np.ascontiguousarray(textfile.read_tap(img)))
    assert rc == -52 and "block sizes" in msg
    items = np.ascontiguousarray(textfile.read_tap(img))
    for field, value, code in (("length", 0, -54), ("length", 131072, -54), ("offset", len(img), -55), ("length", 13, -55), ("kind", 3, -53)):
        bad = items.copy()
        bad[field][0] = value
        rc, msg, _ = fmt(img, TextOptions("hex"), items=bad)
        assert rc == code, (field, value, rc, msg)
    o = textfile.c_options(TextOptions("hex"))
    for k, v in ((0, 4), (1, 13), (2, 3), (2, 401), (3, 401)):
        d = (C.c_int * 7)(o.numtype, o.chartype, o.linesize, o.dataspace, o.linefeed, o.ntrks, 0)
        d[k] = v
        assert fmt.lib.rtfe_text_format_scratch_bytes(None, 0, 0, d) == 0 and "out of range" in fmt.lib.rtfe_last_error().decode()
