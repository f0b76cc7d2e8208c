"""The part of torch.distributed that readtape_amd/shard.py uses, in ONE process: N threads are N ranks (test infrastructure only).

A single-GPU machine cannot host two RCCL ranks, but it can run N threads, each with its own FrontEnd, its own rows and its own place in the
collectives: the halo-growing loop, the ownership rule, the per-rank replay and the gather of shard.decode_sharded / decode_file_sharded then run
against the real kernels with one process holding the GPU.  Tensors are copied between the ranks' tensors as they are given, on any device.

    results = local_group.run(3, lambda rank, dist: shard.decode_file_sharded(path, tap, rank, 3, dist))

Every wait has a timeout, and a rank that raises breaks the group: the other threads raise too, so a test fails where it would have hung.
What this is NOT: RCCL, several processes, several devices, overlap of communication with anything."""
from __future__ import annotations

import threading

# Only turns a hang into a failure.  The slowest test that uses the group (tests/test_gpu_shard_file.py::test_goldens[nrzi9_nobpi-3]: the first one, three
# ranks, the density detection on rank 0 while the other two wait in the broadcast) was observed at 0.33 s on an MI355X, every other one below 0.1 s.
TIMEOUT = 120.0


class GroupBroken(RuntimeError):
    """Another rank raised (or a wait timed out): this rank stops with it."""


class ReduceOp:
    MAX = "max"
    MIN = "min"


class _Work:
    def __init__(self, group):
        self.group, self.done = group, False

    def wait(self):
        self.group._wait(lambda: self.done, "a send or receive whose partner never came")


class P2POp:
    def __init__(self, op, tensor, peer):
        self.op, self.tensor, self.peer = op, tensor, peer


class _Group:
    def __init__(self, world, timeout):
        self.world, self.timeout = int(world), float(timeout)
        self.cv = threading.Condition()
        self.broken = None
        self.gen, self.count, self.slots, self.results, self.readers = 0, 0, [None] * self.world, {}, {}
        self.sends, self.recvs = {}, {}                    # (src, dst) -> [(tensor, work)] posted and not yet matched, in order

    def _break(self, why):
        with self.cv:
            if self.broken is None:
                self.broken = why
            self.cv.notify_all()

    def _wait(self, pred, what):
        """with the lock held or not: waits until pred() holds; raises when the group is broken or the timeout runs out"""
        with self.cv:
            self.cv.wait_for(lambda: pred() or self.broken is not None, self.timeout)
            if pred():                                       # (what it waited for has come: a rank that raised behind it does not undo that)
                return
            if self.broken is not None:
                raise GroupBroken(f"local_group: {self.broken}")
            self.broken = f"timeout after {self.timeout:.0f} s waiting for {what}"
            self.cv.notify_all()
            raise GroupBroken(f"local_group: {self.broken}")

    def exchange(self, rank, item):
        """every rank gives an item and gets the list of all ranks' items (a barrier)"""
        with self.cv:
            gen = self.gen
            self.slots[rank] = item
            self.count += 1
            if self.count == self.world:
                self.results[gen], self.readers[gen] = self.slots, self.world
                self.slots, self.count, self.gen = [None] * self.world, 0, gen + 1
                self.cv.notify_all()
            self._wait(lambda: gen in self.results, "the other ranks in a collective")
            out = self.results[gen]
            self.readers[gen] -= 1
            if self.readers[gen] == 0:
                del self.results[gen], self.readers[gen]
            return out

    def post(self, kind, src, dst, tensor):
        """a send or a receive: whichever side comes second copies, so no order of posting or waiting can deadlock"""
        work = _Work(self)
        with self.cv:
            mine, theirs = (self.sends, self.recvs) if kind == "send" else (self.recvs, self.sends)
            q = theirs.get((src, dst))
            if q:
                other, other_work = q.pop(0)
                s, r = (tensor, other) if kind == "send" else (other, tensor)
                if tuple(s.shape) != tuple(r.shape) or s.dtype != r.dtype:
                    self.broken = f"send {tuple(s.shape)} {s.dtype} from rank {src} meets receive {tuple(r.shape)} {r.dtype} on rank {dst}"
                    self.cv.notify_all()
                    raise GroupBroken(f"local_group: {self.broken}")
                _copy(r, s)
                work.done = other_work.done = True
                self.cv.notify_all()
            else:
                mine.setdefault((src, dst), []).append((tensor, work))
        return work


def _copy(dst, src):
    dst.copy_(src)
    if dst.is_cuda or src.is_cuda:                           # (the ranks share the device's streams here; the data are there before anyone is told so)
        import torch
        torch.cuda.synchronize()


class Dist:
    """One rank's view of the group: pass it where shard.py takes `dist`."""
    ReduceOp = ReduceOp
    P2POp = P2POp

    def __init__(self, group, rank):
        self._g, self.rank = group, int(rank)

    def _collective(self, tensor, fill):
        """all ranks' tensors -> fill(them) writes this rank's outputs; nobody leaves while someone still reads"""
        them = self._g.exchange(self.rank, tensor)
        fill(them)
        self._g.exchange(self.rank, None)

    def all_reduce(self, tensor, op=ReduceOp.MAX):
        import torch
        them = self._g.exchange(self.rank, tensor)
        acc = them[0].clone()
        for t in them[1:]:
            acc = torch.maximum(acc, t.to(acc.device)) if op == ReduceOp.MAX else torch.minimum(acc, t.to(acc.device))
        self._g.exchange(self.rank, None)                    # (everyone has read the inputs before anyone overwrites its own)
        _copy(tensor, acc)

    def all_gather(self, out, tensor):
        self._collective(tensor, lambda them: [_copy(o, t) for o, t in zip(out, them)])

    def gather(self, tensor, gather_list=None, dst=0):
        self._collective(tensor, lambda them: [_copy(o, t) for o, t in zip(gather_list, them)] if self.rank == dst else None)

    def broadcast(self, tensor, src=0):
        self._collective(tensor, lambda them: _copy(tensor, them[src]) if self.rank != src else None)

    def isend(self, tensor, dst):
        return self._g.post("send", self.rank, dst, tensor)

    def irecv(self, tensor, src):
        return self._g.post("recv", src, self.rank, tensor)

    def batch_isend_irecv(self, ops):
        return [self.isend(o.tensor, o.peer) if o.op.__name__ == "isend" else self.irecv(o.tensor, o.peer) for o in ops]


def run(world, fn, timeout=TIMEOUT, raise_first=True):
    """fn(rank, dist) on `world` threads -> [each rank's result].  A rank that raises breaks the group (the others raise GroupBroken in their next
    wait); the first error in time that is not a GroupBroken is raised again - or, with raise_first=False, every rank's result or exception is returned."""
    group = _Group(world, timeout)
    out, order = [None] * world, []

    def body(rank):
        try:
            out[rank] = fn(rank, Dist(group, rank))
        except BaseException as e:
            out[rank] = e
            order.append(rank)
            group._break(f"rank {rank} raised {type(e).__name__}: {e}")

    threads = [threading.Thread(target=body, args=(r,), name=f"local-rank-{r}") for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if raise_first and order:
        real = [r for r in order if not isinstance(out[r], GroupBroken)] or order
        raise out[real[0]]
    return out
