"""A plain statement of the quiet map and the burst table (what k_quiet, k_sift / k_qpack, k_dseg and k_bursts* write), in numpy and Python integers,
written from the contract in include/rt_frontend.h and the comments of rtfe_api.hip / rtfe_kernels.hip - lists of group numbers, no words, no bit tricks.

Which fields of rtfe_burst are compared, and why
  Of an OWNED burst (index < nbursts) the kernels behind the table - k_zones / k_publish, the chains, k_decode, k_zeros, k_diffz - replace reset_sample,
  safe_last and end_sample by the restart rows they decide, and OR their own conditions into flags; they read zone_first, zone_end, event_base and
  event_cap and never write them.  So of an owned burst
      zone_first, zone_end, event_base, event_cap            are compared as they are, and
      flags & (EXACT_START | EVENT_OVERFLOW | TRUNCATED)     - the three bits k_bursts* sets.  (UNSAFE, SCREEN_UNDERFLOW, DETECTOR_FATAL, AGC_FATAL and
                                                               STATE_AT_END belong to the detectors.  EVENT_OVERFLOW is shared: a detector sets it when a
                                                               list outgrows event_cap - the test tapes hold a few isolated samples, a handful of events a
                                                               burst at the most against a capacity of 64 or more, or a capacity of 0 that k_bursts* flagged
                                                               already - so on these tapes the bit is k_bursts*'s alone.)
  Time shards: the table entry at index nbursts is the first burst of the right neighbour, which only bounds the last owned one.  No later kernel touches it,
  so ALL of its fields are compared: reset_sample = safe_last = -1 and the provisional end_sample included.
  nbursts, and the count of entries with the bounding one (BurstScratch::nbursts_total, the third int of the workspace), are compared too.
  reset_sample, safe_last and end_sample of owned bursts are k_zones' and the detectors' business and are not looked at here."""
import numpy as np

F_EXACT_START, F_EVENT_OVERFLOW, F_TRUNCATED = 1, 4, 32
OWNED_FLAGS = F_EXACT_START | F_EVENT_OVERFLOW | F_TRUNCATED
GROUP = 64            # rows of a group of the quiet map
MARGIN = 256          # rows in front of zone_end that a burst's extent starts at (kMarginRows)
OWNED_FIELDS = ("zone_first", "zone_end", "event_base", "event_cap")
ALL_FIELDS = ("zone_first", "zone_end", "reset_sample", "safe_last", "end_sample", "event_base", "event_cap")


def derive(cfg):
    """quiet_i, gap_chunks and cap_frac as rtfe_create derives them from a configuration (rtfe_api.hip)."""
    f32 = np.float32
    spb = int(f32(1) / (f32(cfg.bpi) * f32(cfg.ips) * (f32(cfg.tdelta_ns) / f32(1e9))))
    quiet_v = min(f32(max(f32(p[2]), f32(p[1]) / f32(2))) for p in cfg.parmsets)      # a fresh detector sees nothing below min_peak, or below half the rise
    if cfg.find_zeros:
        quiet_v = f32(0.2)
        if cfg.differentiate:
            quiet_v = f32(0.24) / f32(max(spb, 1))
    elif cfg.differentiate:
        quiet_v = min(quiet_v, f32(0.024))
    if 0 < cfg.quiet_volts and f32(cfg.quiet_volts) < quiet_v:
        quiet_v = f32(cfg.quiet_volts)
    lsb_per_volt = 32767.0 / float(f32(cfg.maxvolts))
    quiet_i = max(int(np.floor(float(quiet_v) * 0.98 * lsb_per_volt)) - 1, 0)
    gap = cfg.gap_min_samples if cfg.gap_min_samples > 0 else 32 * max(spb, 1)
    gap = max(gap, MARGIN + 128)
    gap_chunks = (gap + GROUP - 1) // GROUP + 1
    cap_frac = f32(cfg.events_per_sample_cap) if cfg.events_per_sample_cap > 0 else f32(0.125)
    return quiet_i, gap_chunks, cap_frac


def loud_groups_of_rows(rows, quiet_i):
    """The complete groups of 64 rows that hold a sample outside [-quiet_i, quiet_i], ascending."""
    n = rows.shape[0] // GROUP
    x = rows[: n * GROUP].astype(np.int32).reshape(n, -1)
    return np.flatnonzero((np.abs(x) > quiet_i).any(axis=1)).tolist()


def loud_groups_of_pokes(pokes, nrows, quiet_i):
    """The same from the samples poked into an all-zero tape ((row, track, value)); rows of the incomplete last group do not count."""
    n = nrows // GROUP
    return sorted({r // GROUP for r, t, v in pokes if abs(int(v)) > quiet_i and r // GROUP < n})


def zones(loud, ngroups, gap_chunks):
    """Maximal runs of quiet complete groups of at least gap_chunks groups, as (first group, one past the last group)."""
    out, c0 = [], 0
    for g in list(loud) + [ngroups]:          # a run ends in front of a loud group, or with the map (the incomplete last group is not quiet)
        if g - c0 >= gap_chunks:
            out.append((c0, g))
        c0 = g + 1
    return out


def table(loud, nrows, gap_chunks, cap_frac, nparm, ntrks, first_is_tape_start, own_rows, event_capacity, max_bursts):
    """The burst table k_bursts* leaves: a list of dicts, bounding entry included, and (nbursts, nbursts_total).
    Every entry also carries cap_f64, the capacity a double product would have given (for the shapes that aim at the float32 rounding)."""
    ngroups = nrows // GROUP
    zs = zones(loud, ngroups, gap_chunks)
    ent = []
    begins_in_zone = bool(zs) and zs[0][0] == 0
    if first_is_tape_start and not begins_in_zone:
        ent.append(dict(zone_first=0, zone_end=0, reset_sample=0, safe_last=0, flags=F_EXACT_START))
    for c0, c1 in zs:
        # zone_end = 64 * c1 never passes the last complete group, so the kernel's clamp (zone_end > nrows -> nrows rounded down to 64) never engages:
        # a zone that ends with the map ends at nrows rounded down to a multiple of 64 either way
        assert GROUP * c1 <= nrows
        ent.append(dict(zone_first=GROUP * c0, zone_end=GROUP * c1, reset_sample=-1, safe_last=-1, flags=0))
    assert len(ent) <= max_bursts, "the shape outgrows the table: not what these tests are about"
    # Ownership between time shards.  The right neighbour's row 0 is this scan's own_rows.  A zone that reaches gap_chunks groups or more past own_rows shows the
    # neighbour a qualifying zone of its own, so the neighbour decodes the burst behind it; a zone that ends earlier shows the neighbour too few quiet groups
    # and stays here.  The first burst that is the neighbour's only bounds the last owned one; everything behind it is dropped.  An exact-start burst is row 0's
    # and always owned.
    n_owned = len(ent)
    if own_rows < nrows:
        for b, e in enumerate(ent):
            if not (e["flags"] & F_EXACT_START) and e["zone_end"] >= own_rows + gap_chunks * GROUP:
                n_owned = b
                break
    ent = ent[: n_owned + 1]
    lists = nparm * ntrks
    base = 0
    for b, e in enumerate(ent):
        start = 0 if e["flags"] & F_EXACT_START else e["zone_end"] - MARGIN
        end = ent[b + 1]["zone_end"] if b + 1 < len(ent) else nrows
        length = max(end - start, 0)
        cap = int(np.float32(length) * np.float32(cap_frac)) + 64
        e["cap_f64"] = int(float(length) * float(cap_frac)) + 64
        e["end_sample"] = end
        e["event_base"], e["event_cap"] = base, cap
        if base + cap * lists > event_capacity:          # the region would pass the arena: no room at all, flagged; the bases go on as if it had fitted
            e["event_cap"] = 0
            e["flags"] |= F_EVENT_OVERFLOW
        base += GROUP * ((cap * lists + GROUP - 1) // GROUP)
    if n_owned == len(ent) and own_rows < nrows and n_owned > 0:          # the halo holds no further zone
        ent[n_owned - 1]["flags"] |= F_TRUNCATED
    return ent, n_owned, len(ent)


def pack_plan(counts, event_caps):
    """rtfe_pack_events' plan for a scan's list counts [nbursts, lists]: per burst its longest list (at least 1, at most the region), the packed bases, the total."""
    cap2, bases, total = [], [], 0
    lists = counts.shape[1]
    for b in range(counts.shape[0]):
        c = min(max(int(counts[b].max()), 1), int(event_caps[b]))
        cap2.append(c)
        bases.append(total)
        total += c * lists
    return cap2, bases, total


def compare(ent, n_owned, n_total, bursts, bounding, nbursts_total):
    """Every compared field of every burst, no tolerance: raises AssertionError naming the burst and the field."""
    assert len(bursts) == n_owned, f"nbursts {len(bursts)}, the reference has {n_owned}"
    assert nbursts_total == n_total, f"nbursts_total {nbursts_total}, the reference has {n_total}"
    for b in range(n_owned):
        for k in OWNED_FIELDS:
            assert int(bursts[k][b]) == ent[b][k], f"burst {b} {k}: {int(bursts[k][b])}, the reference has {ent[b][k]}"
        got = int(bursts["flags"][b]) & OWNED_FLAGS
        assert got == ent[b]["flags"], f"burst {b} flags: {got:#x}, the reference has {ent[b]['flags']:#x}"
    if n_total > n_owned:
        assert len(bounding) == 1
        for k in ALL_FIELDS:
            assert int(bounding[k][0]) == ent[n_owned][k], f"bounding burst {k}: {int(bounding[k][0])}, the reference has {ent[n_owned][k]}"
        assert int(bounding["flags"][0]) == ent[n_owned]["flags"], f"bounding burst flags: {int(bounding['flags'][0]):#x}"
