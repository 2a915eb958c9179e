"""The staged-batch pipeline the real-image loaders share, and the pinned upload / copy back of the detectors: DESIGN §23 has the
ordering rules.  A loader adds `_sample`, its layout, its pack and its launch; `hand_over` is the host scheduling alone, no device."""
import os
from concurrent.futures import ThreadPoolExecutor

import torch


def align(n, a=16):
    return (n + a - 1) // a * a


def default_decode(path):
    from PIL import Image
    return Image.open(path).convert("RGB")


def pinned(t, need, step=1 << 20):
    """-> `t`, or a new pinned uint8 tensor when `t` is None or shorter than `need` bytes; sizes grow in `step`s"""
    if t is None or t.numel() < need:
        t = torch.empty(align(max(need, 1), step), dtype=torch.uint8, pin_memory=True)
    return t


class Slot:
    """One pinned staging buffer and the event recorded behind the last H2D copy out of it"""

    def __init__(self):
        self.pinned, self.event = None, None

    def buffer(self, need):
        """-> the pinned buffer, at least `need` bytes, once the previous copy out of it has completed"""
        if self.event is not None:
            self.event.synchronize()
        self.pinned = pinned(self.pinned, need)
        return self.pinned


class Layout:
    """Byte layout of one staged batch; `fills`: [(cache entry, byte offset in the slot)], the whole files that ride behind it"""
    fills = ()


def fills_behind(nbytes, entries):
    """Cache entries seen for the first time go up once, behind a batch of `nbytes` at aligned offsets -> (fills, bytes needed)"""
    fills, need = [], nbytes
    for e in entries:
        fills.append((e, need))
        need = align(need + e.nbytes)
    return fills, need


def copy_fills_host(host, fills):
    for e, at in fills:
        host[at:at + e.nbytes] = e.frame.reshape(-1)


def copy_fills_device(pool, pinned_buf, fills):
    """pinned -> each file's slot of the pool, in front of the batch's kernels"""
    for e, at in fills:
        pool[e.offset:e.offset + e.nbytes].copy_(pinned_buf[at:at + e.nbytes], non_blocking=True)


def hand_over(nb, stage, enqueue, slots, prefetch=True):
    """Yield `enqueue(stage(j, slots[j % 3]))` for j in 0..nb-1, in order.  With `prefetch`, `stage` runs on one stager thread
    up to two batches ahead of the one being enqueued (so slot j % 3 is reused only after batch j - 3 was enqueued); without, inline.
    A generator that is abandoned shuts the stager down and cancels what it has not started."""
    stager = ThreadPoolExecutor(1, thread_name_prefix="mdcv-stage") if prefetch else None
    try:
        pending = {}
        for bi in range(nb):
            if prefetch:
                for j in range(bi, min(nb, bi + 3)):
                    if j not in pending:
                        pending[j] = stager.submit(stage, j, slots[j % 3])
            yield enqueue(pending.pop(bi).result() if prefetch else stage(bi, slots[bi % 3]))
    finally:
        if stager is not None:
            stager.shutdown(wait=True, cancel_futures=True)


class StagedBatches:
    """What `ImageLabelBatches` and `ConeCropBatches` share: the slots, the decode pool, the side stream and its ordering, the hand-over"""

    def _init_staging(self, num_workers, decode, prefetch, device, cache=None):
        self.num_workers = int(num_workers) if num_workers is not None else max(1, min(16, os.cpu_count() or 1))
        self.decode, self.prefetch = decode or default_decode, bool(prefetch)
        self._device, self._cache = device, cache
        self._pool, self._stream, self._last_ready = None, None, None
        self._slots = [Slot() for _ in range(3)]

    @property
    def device(self):
        if self._device is None:
            return torch.device("cuda", torch.cuda.current_device())
        return torch.device(self._device)

    def cache_stats(self):
        """None without `cache_bytes`; else hits / fills (samples that read the pool without / after decoding their file), misses by
        reason (samples staged the old way), bytes_reserved (by admission) and pool_bytes (allocated, a staging tail included)."""
        return None if self._cache is None else self._cache.stats()

    def _map(self, sample, idx):
        return list(self._pool.map(sample, idx)) if self._pool is not None else [sample(i) for i in idx]

    def _copied(self, slot, fills):
        """behind the H2D copies out of `slot`: the event that frees its pinned buffer and marks the fills' slots written"""
        ev = torch.cuda.Event()
        ev.record(self._stream)
        slot.event = ev
        if self._cache is not None:
            self._cache.filled([e for e, _ in fills], ev)

    def _ready(self):
        """behind a batch's last launch: the event the consumer's stream, and the next epoch's side stream, wait for"""
        self._last_ready = torch.cuda.Event()
        self._last_ready.record(self._stream)
        return self._last_ready

    def _batches(self, nb, stage):
        """One epoch on a new side stream: `stage(j, slot)` then `self._enqueue(staged)` -> (*batch, ready) per batch, yielded without
        `ready` once the consumer's stream waits for it."""
        dev = self.device
        self._stream = torch.cuda.Stream(dev)
        c = self._cache
        if c is not None:
            c.restart()
            if c.pool is None:
                with torch.cuda.device(dev):
                    if c.ensure_pool(dev) is not None:           # allocated on the consumer's stream, written on the side streams
                        self._stream.wait_stream(torch.cuda.current_stream(dev))
            if self._last_ready is not None:                     # the earlier epoch's last work: its fills, its last launch's reads
                self._stream.wait_event(self._last_ready)
        if self.num_workers > 1 and self._pool is None:
            self._pool = ThreadPoolExecutor(self.num_workers, thread_name_prefix="mdcv-decode")

        def enqueue(staged):
            *batch, ready = self._enqueue(staged)
            cons = torch.cuda.current_stream(dev)
            cons.wait_event(ready)
            for t in batch:
                if isinstance(t, torch.Tensor):
                    t.record_stream(cons)
            return tuple(batch)
        return hand_over(nb, stage, enqueue, self._slots, self.prefetch)

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        if self._cache is not None:
            if self._cache.pool is not None and self._stream is not None:
                self._cache.pool.record_stream(self._stream)     # the last epoch's kernels may still read it
            self._cache.close()
            self._last_ready = None


# ---------------------------------------------------------------------------------- the detectors' upload and copy back (one stream)
def upload(pin_in, in_bytes, nbytes, device):
    """-> a fresh device buffer of `nbytes` whose first `in_bytes` are copied from the pinned input"""
    dbuf = torch.empty(nbytes, dtype=torch.uint8, device=device)
    dbuf[:in_bytes].copy_(pin_in[:in_bytes], non_blocking=True)
    return dbuf


def copy_back(dbuf, lo, pin_out, stream):
    """dbuf[lo:] -> pinned memory and the batch's final host synchronisation -> (the pinned buffer, table): `table(off, nbytes, dtype,
    shape)` views the bytes at dbuf offset `off`; the buffer is the next batch's, so a caller copies what it keeps."""
    n = dbuf.numel() - lo
    pin_out = pinned(pin_out, n)
    pin_out[:n].copy_(dbuf[lo:], non_blocking=True)
    done = torch.cuda.Event()
    done.record(stream)
    done.synchronize()
    out = pin_out.numpy()

    def table(off, nbytes, dtype, shape):
        return out[off - lo:off - lo + nbytes].view(dtype).reshape(shape)
    return pin_out, table
