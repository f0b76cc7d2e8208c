"""CPU: shard.plan_file_shards - the ranks' shares of a capture file in used rows and the raw rows each is made of (-subsample, -skip) - against a
brute-force numpy statement; the new keywords of the sharded decode being off by default; and tests/local_group.py, the in-process group the GPU
tests run their ranks on, with CPU tensors."""
import inspect
import time

import numpy as np
import pytest
import torch

import local_group
from readtape_amd import ingest, shard

RAW = (0, 1, 1023, 1024, 20204, 94586, (1 << 20) + 5)


@pytest.mark.parametrize("align", [64, 1024])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_every_used_row_has_one_owner_and_its_group_of_raw_rows(n, align):
    seen_empty = 0
    for raw in RAW:
        for skip in (0, 1, 1531, raw + 7):
            # the statement: raw row r is used iff it lies behind the skip and is the last of its group of n; used row j is the j-th of them
            r = np.arange(raw, dtype=np.int64)
            used_raw = r[(r >= skip) & ((r - skip) % n == n - 1)]
            used = used_raw.shape[0]
            assert used == max(0, raw - skip) // n
            for world in range(1, 9):
                tag = (raw, skip, n, world, align)
                plan = shard.plan_file_shards(raw, world, n, skip, align)
                assert len(plan) == world, tag
                assert [(p[0], p[1]) for p in plan] == shard.plan_shards(used, world, align), tag
                assert plan[0][0] == 0 and plan[-1][1] == used, tag
                owner = np.full(used, -1)
                for k, (lo, hi, raw_lo, raw_hi) in enumerate(plan):
                    assert 0 <= lo <= hi <= used, tag
                    assert lo == (plan[k - 1][1] if k else 0), tag                         # contiguous
                    assert lo % align == 0 or lo == used, tag                              # on the grid
                    assert raw_hi <= raw or hi == lo, tag                                  # nothing behind the payload
                    # the raw range holds exactly the groups of the rank's used rows: its used rows are the rank's, thinned as the kernel thins them
                    mine = r[raw_lo:raw_hi][n - 1::n]
                    assert (mine == used_raw[lo:hi]).all() and raw_hi - raw_lo == (hi - lo) * n, tag
                    assert (owner[lo:hi] == -1).all()
                    owner[lo:hi] = k
                    if hi == lo:
                        assert (lo, hi) == (used, used) and all(p[0] == p[1] == used for p in plan[k:]), tag      # empty ranks are the last ones
                        seen_empty += 1
                assert (owner >= 0).all(), tag
                if used < world * align and world > 1:
                    assert plan[-1][0] == plan[-1][1] == used, tag                         # a tape too short for the ranks
    assert seen_empty > 20


def test_bad_options_are_refused():
    for kw in (dict(subsample=0), dict(skip=-1)):
        with pytest.raises(ValueError):
            shard.plan_file_shards(1000, 2, **kw)


def test_the_options_are_off_by_default():
    """The new keywords of the sharded decodes and of the pre-passes (off: their present callers see no change)."""
    sig = inspect.signature(shard.decode_sharded).parameters
    assert list(sig)[:12] == ["hdr", "own", "lo", "n_total", "rank", "world", "dist", "tap_path", "opts", "fe_factory", "halo_rows", "cfgkw"]
    assert [sig[k].default for k in ("opts", "fe_factory", "halo_rows", "cfgkw", "deskew", "skew")] == [None, None, 1 << 16, None, False, None]
    sig = inspect.signature(shard.decode_file_sharded).parameters
    assert list(sig) == ["path", "tap_path", "rank", "world", "dist", "opts", "cfgkw", "halo_rows", "subsample", "skip", "deskew", "skew", "prepass_rows",
                         "device", "align", "fe_factory", "_lib_path", "_backend"]
    assert [sig[k].default for k in list(sig)[5:]] == [None, None, 1 << 16, 1, 0, False, None, 1 << 22, "cuda:0", 1024, None, None, None]
    sig = inspect.signature(shard.plan_file_shards).parameters
    assert [sig[k].default for k in ("subsample", "skip", "align")] == [1, 0, 1024]
    sig = inspect.signature(ingest._prepasses).parameters
    assert [sig[k].default for k in ("fe_factory", "backend", "lib")] == [None, None, None]


# ---- the in-process group ----

def test_halo_exchange_among_three_ranks_equals_slicing():
    """shard.exchange_halo over local_group: every rank's rows with halo are the tape's rows [lo, hi + halo) - a halo that spans two ranks included."""
    rng = np.random.default_rng(3)
    tape = torch.from_numpy(rng.integers(-3000, 3000, (5000, 9)).astype(np.int16))
    spans = [(0, 2048), (2048, 2688), (2688, 5000)]
    for halo in (100, 640, 1500, 9000):
        def rank_fn(rank, dist):
            lo, hi = spans[rank]
            rows, own = shard.exchange_halo(tape[lo:hi].clone(), halo, rank, 3, dist)
            return rows.clone(), own
        for rank, (rows, own) in enumerate(local_group.run(3, rank_fn, timeout=60)):
            lo, hi = spans[rank]
            assert own == hi - lo and torch.equal(rows, tape[lo: min(5000, hi + halo)]), (halo, rank)


def test_the_collectives_equal_their_definitions():
    def rank_fn(rank, dist):
        t = torch.tensor([rank, 10 - rank, 7], dtype=torch.int64)
        mx, mn = t.clone(), t.clone()
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        dist.all_reduce(mn, op=dist.ReduceOp.MIN)
        ag = [torch.zeros_like(t) for _ in range(4)]
        dist.all_gather(ag, t)
        g = [torch.zeros_like(t) for _ in range(4)] if rank == 2 else None
        dist.gather(t, g, dst=2)
        b = t.clone()
        dist.broadcast(b, src=1)
        return mx.tolist(), mn.tolist(), [x.tolist() for x in ag], None if g is None else [x.tolist() for x in g], b.tolist(), shard.gather_lens(rank * 3, "cpu", 4, dist)
    every = [[r, 10 - r, 7] for r in range(4)]
    for rank, (mx, mn, ag, g, b, lens) in enumerate(local_group.run(4, rank_fn, timeout=60)):
        assert mx == [3, 10, 7] and mn == [0, 7, 7] and ag == every and b == [1, 9, 7] and lens == [0, 3, 6, 9]
        assert g == (every if rank == 2 else None)


def test_sends_and_receives_match_in_any_order_of_waiting():
    """Two ranks send to each other and wait for their sends first: whoever posts second copies, nobody waits for a wait."""
    def rank_fn(rank, dist):
        out, inn = torch.full((4,), rank + 1), torch.zeros(4, dtype=torch.int64)
        works = dist.batch_isend_irecv([dist.P2POp(dist.isend, out, 1 - rank), dist.P2POp(dist.irecv, inn, 1 - rank)])
        for w in works:
            w.wait()
        return inn.tolist()
    assert local_group.run(2, rank_fn, timeout=60) == [[2] * 4, [1] * 4]


def test_a_raising_rank_stops_the_others_within_the_timeout():
    def rank_fn(rank, dist):
        t = torch.zeros(1, dtype=torch.int64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        if rank == 1:
            raise KeyError("injected")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)             # (rank 1 never comes)
        return "left the collective"
    t0 = time.perf_counter()
    out = local_group.run(3, rank_fn, timeout=60, raise_first=False)
    assert time.perf_counter() - t0 < 30
    assert isinstance(out[1], KeyError) and all(isinstance(out[r], local_group.GroupBroken) and "rank 1 raised KeyError" in str(out[r]) for r in (0, 2))
    with pytest.raises(KeyError, match="injected"):          # (the first error that is not the group's own)
        local_group.run(3, rank_fn, timeout=60)
