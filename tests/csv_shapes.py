"""CSV texts and window cuts aimed at the seams of the device CSV path (readtape_amd/csrc/rtfe_csv.hip, csvin.read_csv_device): the number and line
shapes the byte loops of csrc/host/rt_csv.c decide, newlines at the edges of a lane's 16 bytes and of a workgroup's 4 KB, waves on either side of the
LDS budget, windows cut at every kind of byte, the pre-read's cut-off.  The kernel constants the shapes depend on are mirrored here and asserted
against the source (check_constants).  Test infrastructure."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE_BYTES, BLOCK_BYTES, WAVE_LINES, LDS_BUDGET = 16, 4096, 64, 8192


def check_constants():
    src = open(os.path.join(ROOT, "readtape_amd", "csrc", "rtfe_csv.hip")).read()
    got = {k: int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("kCsvLaneBytes", "kCsvBlockBytes", "kCsvWaveLines", "kCsvLdsBudget")}
    assert got == dict(kCsvLaneBytes=LANE_BYTES, kCsvBlockBytes=BLOCK_BYTES, kCsvWaveLines=WAVE_LINES, kCsvLdsBudget=LDS_BUDGET), got
    assert "e1 - a0 > (uint32_t)kCsvLdsBudget" in src and "starts[first_line + j0] & ~15u" in src      # wave_branches below restates these
    host = open(os.path.join(ROOT, "readtape_amd", "csrc", "host", "rt_csv.c")).read()
    assert "LINE_MAX_CHARS = 400" in host


def titles(ntrks=9):
    return [b"Saleae export\n", ("Time [s], " + ", ".join(f"c{k}" for k in range(ntrks)) + "\n").encode()]


def values(n, ntrks, seed=1, amp=3.0):
    rng = np.random.RandomState(seed)
    t = np.arange(n)[:, None]
    return amp * np.sin(0.37 * t + np.arange(ntrks)[None, :]) + rng.uniform(-0.3, 0.3, (n, ntrks))


def data_line(i, vals, dt=1.28e-6, t0=0.0125):
    return (f"{t0 + i * dt:.9f}, " + ", ".join(f"{v:.6f}" for v in vals) + "\n").encode()


def plain_lines(n, ntrks=9, seed=1, amp=3.0):
    v = values(n, ntrks, seed, amp)
    return [data_line(i, v[i]) for i in range(n)]


def padded(line, length):
    """The line made `length` bytes long ('\\n' included) by blanks behind its first comma: blanks in front of a number are skipped."""
    assert line.endswith(b"\n") and len(line) <= length, (len(line), length)
    k = line.index(b",") + 1
    return line[:k] + b" " * (length - len(line)) + line[k:]


def shape(name, lines, ntrks=9, windows=(1 << 20, 1000), head=None, path="device", preread=None, **kw):
    text = b"".join((head if head is not None else titles(ntrks)) + list(lines))
    return dict(name=name, text=text, kw=dict(ntrks=ntrks, **kw), windows=list(windows), path=path, preread=preread)


def window_cuts(text, window_bytes):
    """The file offsets at which read_csv_device's windows end (each window: the bytes carried from the one before, filled up to window_bytes)."""
    cuts, pos, carry = [], 0, 0
    while pos < len(text):
        n = min(window_bytes - carry, len(text) - pos)
        start, pos = pos - carry, pos + n
        cuts.append(pos)
        if pos >= len(text):
            break
        nl = text.rfind(b"\n", start, pos)
        assert nl >= start, "a line longer than the window"
        carry = pos - (nl + 1)
    return cuts


def wave_branches(text, first_line=2):
    """For the file as ONE window: per wave of 64 lines from first_line on, True where k_csv_parse / k_csv_peak stage the wave's span into LDS."""
    starts = [0] + [i + 1 for i in range(len(text)) if text[i:i + 1] == b"\n"]
    if not text.endswith(b"\n"):
        starts.append(len(text))
    nlines = len(starts) - 1
    out = []
    for j0 in range(first_line, nlines, WAVE_LINES):
        j1 = min(j0 + WAVE_LINES, nlines)
        out.append(starts[j1] - (starts[j0] & ~15) <= LDS_BUDGET)
    return out


def number_shapes():
    z = "0.000000"
    rows = []

    def row(i, fields, sep=", "):
        rows.append((f"{0.001 + i * 1e-6:.7f}" + sep + sep.join(fields) + "\n").encode())
    row(0, ["3", "-2", "-.5", ".25", "-0.000000", "7.", "-4", "0", "1"])                                          # no fraction, no integer part, minus zero
    row(1, ["0.12345678901234567890", "1.23456789012", "2.3456789012345", "-3.456789012345678", "0.999999999999", "1.0000000000001", "9.87654321098765", "0.33333333333333333333", "-1.99999999999999999999"])
    row(2, ["0." + "123456789" * 5, "-0." + "9" * 45, "1." + "0" * 44 + "9", z, z, z, z, z, z])                     # 45 fraction digits: scale overflows to inf
    row(3, ["-", "1.5", "2.5", "-", z, z, z, z, "-"])                                                              # a field of only '-': stops nothing, reads -0
    rows.append(b"0.0010040 ,  1.5 ,2.5  ,   -3.5 , 0.5,,1.25 ,-0.75,  2.0,3.0 \n")                                # blanks before and after commas, an empty field
    row(5, ["1e3", "2.5", z, z, z, z, z, z, z])                                                                    # an 'e' stops the field and every field behind it
    row(6, ["1.5", "2\t.5", "3.5", z, z, z, z, z, z])                                                              # a tab
    rows.append(b"0.0010070, 1.5, 2.5\0, 3.5, 1, 1, 1, 1, 1, 1\n")                                                 # a NUL byte
    row(8, ["1.5", "-2.5"])                                                                                       # a short line: missing fields stay 0
    row(9, ["0.1", "0.2", "0.3", "0.4", "0.5", "0.6", "0.7", "0.8", "0.9", "5.5", "6.5"])                          # extra fields
    rows.append(b"\n")                                                                                            # a blank line in the middle
    row(11, ["+1.5", "2.5", z, z, z, z, z, z, z])                                                                  # a '+' is no part of a number
    row(12, ["-1.25"] * 9)
    out = [shape("numbers", rows, windows=(1 << 20, 450, 401)),
           shape("numbers_scale_invert", rows, scale=0.5, invert=True, windows=(1 << 20, 512)),
           shape("numbers_given_maxvolts", rows, maxvolts=20.0, windows=(1 << 20, 600))]
    big = list(rows)
    big.insert(2, (b"0.0010015, 123456789012, 1, 2, 3, 4, 5, 6, 7, 8\n"))                                          # twelve integer digits: the survey's (int) overflows on the host
    out.append(shape("numbers_int_overflow", big, windows=(1 << 20, 700)))
    crlf = [ln[:-1] + b"\r\n" for ln in plain_lines(20)]
    out.append(shape("crlf", crlf, head=[b"Saleae export\r\n", b"Time [s], a, b, c, d, e, f, g, h, i\r\n"], windows=(1 << 20, 333)))
    # clipping on both rails, a code of exactly +-32767 (counts as clipped) and one code inside it: full scale 4.0 given, the surveyed lines below it
    lines = plain_lines(60, amp=2.0)
    inside = 4.0 * 32766 / 32767
    lines[52] = data_line(52, [4.0, -4.0, inside, -inside, 9.5, -9.5, 4.01, -4.01, 0.0])
    lines[57] = data_line(57, [7.0] * 9)
    out.append(shape("clip_rails", lines, maxvolts=4.0, preread=50, windows=(1 << 20, 777)))
    out.append(shape("clip_rails_invert", lines, maxvolts=4.0, invert=True, preread=50, windows=(1 << 20, 777)))
    out.append(shape("perm7", plain_lines(70, ntrks=7, seed=3), ntrks=7, order="543210p", windows=(1 << 20, 900)))
    out.append(shape("perm7_sub2_invert", plain_lines(71, ntrks=7, seed=4), ntrks=7, order="p012345", subsample=2, invert=True, scale=0.5, windows=(1 << 20, 640)))
    return out


def line_shapes():
    out = []
    base = plain_lines(30)
    out.append(shape("no_final_newline", base[:-1] + [base[-1][:-1]], windows=(1 << 20, 500)))
    out.append(shape("titles_only", [], windows=(1 << 20, 64)))
    out.append(shape("titles_only_unterminated", [], head=[b"a\n", b"t, x, y"], windows=(1 << 20, 16)))
    out.append(shape("one_data_line", base[:1], windows=(1 << 20, 120)))
    out.append(shape("two_data_lines", base[:2], windows=(1 << 20, 120)))
    for n in (1, 7, 19):
        out.append(shape(f"ntrks{n}", plain_lines(40, ntrks=n, seed=10 + n), ntrks=n, windows=(1 << 20, 512)))
    for length, path in ((398, "device"), (399, "device"), (400, "host"), (450, "host")):
        lines = plain_lines(12, seed=length)
        lines[5] = padded(lines[5], length)
        out.append(shape(f"line{length}", lines, path=path, windows=(1 << 20, 1024)))
    lines = plain_lines(12, seed=5)
    out.append(shape("line399_unterminated", lines[:-1] + [padded(lines[-1], 400)[:-1]], windows=(1 << 20, 2048)))
    out.append(shape("line400_unterminated", lines[:-1] + [padded(lines[-1], 401)[:-1]], path="host", windows=(1 << 20, 2048)))
    out.append(shape("title_450", lines, head=[b"x" * 449 + b"\n", titles()[1]], path="host", windows=(1 << 20, 2048)))
    out.append(shape("line_longer_than_window", lines, path="host", windows=(100,)))
    out.append(shape("negative_first_time", [b"-" + ln for ln in lines], path="host", windows=(1 << 20,)))
    return out


def seam_shapes():
    out = []
    # a '\n' at byte 15 of a lane's chunk (the first title line: 16 bytes) and at byte 0 of the next but one (the second: 17 bytes)
    lines = plain_lines(20, seed=7)
    out.append(shape("nl_byte15_byte16", lines, head=[b"0123456789abcde\n", b"t,a,b,c,d,e,f,g,h\n"[:16] + b"\n"], windows=(1 << 20, 640)))
    assert out[-1]["text"][15:16] == b"\n" and out[-1]["text"][32:33] == b"\n"
    # a '\n' as the last byte of a 4 KB block and (a blank line) as the first byte of the next
    lines = plain_lines(60, seed=8)
    text, k = b"".join(titles()), 0
    while len(text) + len(lines[k]) + len(lines[k + 1]) < BLOCK_BYTES:
        text += lines[k]
        k += 1
    fill = padded(lines[k], BLOCK_BYTES - len(text))
    body = lines[:k] + [fill, b"\n"] + lines[k + 1:]
    out.append(shape("nl_block_edges", body, windows=(1 << 20, 4096, 4097)))
    assert out[-1]["text"][BLOCK_BYTES - 1: BLOCK_BYTES + 1] == b"\n\n"
    for n in (63, 64, 65, 255, 256, 257):
        out.append(shape(f"lines{n}", plain_lines(n, seed=n), windows=(1 << 20, 3000)))
    for sub, n in ((2, 65), (3, 64), (3, 200), (2, 129)):
        out.append(shape(f"sub{sub}_lines{n}", plain_lines(n, seed=sub * n), subsample=sub, windows=(1 << 20, 1500, 999)))
    # the first window's cut on a '\n', just behind it, on a '-', on a '.', inside the digits of a value and inside the time field
    lines = plain_lines(40, seed=9, amp=2.0)
    lines[9] = data_line(9, [-1.5, 2.25, -0.125, 3.0, -2.0, 1.0, -1.0, 0.5, -0.5])
    sh = shape("cuts", lines, windows=())
    text = sh["text"]
    at = text.index(lines[9])
    cuts = dict(newline=at + len(lines[9]) - 1, behind_newline=at + len(lines[9]), minus=at + lines[9].index(b"-"), point=at + lines[9].index(b".", 14),
                digits=at + lines[9].index(b"2.25") + 3, time=at + 5)
    assert text[cuts["newline"]: cuts["newline"] + 1] == b"\n" and text[cuts["minus"]: cuts["minus"] + 1] == b"-" and text[cuts["point"]: cuts["point"] + 1] == b"."
    for w in cuts.values():
        assert window_cuts(text, w)[0] == w
    sh["windows"] = sorted(cuts.values())
    sh["cut_names"] = cuts
    out.append(sh)
    # windows that hold exactly one line each: every line of the file as long as the window
    lines = [padded(ln, 112) for ln in plain_lines(25, seed=11)]
    out.append(shape("one_line_windows", lines, head=[padded(b"t," + b"x" * 20 + b"\n", 112), padded(titles()[1], 112)], windows=(112, 113, 224)))
    assert window_cuts(out[-1]["text"], 112) == list(range(112, 27 * 112 + 1, 112))
    # waves on either side of the LDS budget: 64 lines of 128 bytes are the budget exactly when the first starts on a 16-byte boundary
    def budget(name, head_len, second, want):
        head = [b"h" * (head_len - 49) + b"\n", padded(titles()[1], 48)]
        lines = [padded(ln, 128) for ln in plain_lines(64, seed=12)] + [padded(ln, second) for ln in plain_lines(64, seed=13)] + plain_lines(2, seed=14)
        sh = shape(name, lines, head=head, windows=(1 << 20,))
        assert len(b"".join(head)) == head_len and wave_branches(sh["text"]) == want, (name, wave_branches(sh["text"]))
        sh["branches"] = want
        out.append(sh)
    budget("lds_at_budget", 96, 128, [True, True, True])
    budget("lds_over_budget", 97, 128, [False, False, True])
    budget("lds_neighbours_differ", 97, 120, [False, True, True])
    budget("lds_neighbours_differ_2", 96, 129, [True, False, True])
    # the pre-read's cut-off at 50: the line on which it stops is counted, not surveyed
    for n in (49, 50, 51, 200):
        out.append(shape(f"preread50_lines{n}", plain_lines(n, seed=100 + n), preread=50, windows=(1 << 20, 2000)))
    for name, at in (("tallest_last_surveyed", 48), ("tallest_first_unsurveyed", 49)):
        lines = plain_lines(120, seed=20, amp=2.0)
        lines[at] = data_line(at, [0.5, -6.75, 0.25, 0, 0, 0, 0, 0, 1.0])
        out.append(shape(f"preread50_{name}", lines, preread=50, windows=(1 << 20, 2500)))
    return out


def all_shapes():
    return number_shapes() + line_shapes() + seam_shapes()


def index_reference(text, is_last):
    """rtfe_csv_index restated: (starts, lines, consumed, longest)."""
    ends = [i + 1 for i in range(len(text)) if text[i:i + 1] == b"\n"]
    starts = [0] + ends + ([len(text)] if is_last and (ends[-1] if ends else 0) < len(text) else [])
    return starts, len(starts) - 1, starts[-1], max([b - a for a, b in zip(starts, starts[1:])], default=0)
