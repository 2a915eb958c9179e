"""Device-resident frame cache: each admitted file is decoded once in a loader's lifetime and its bytes stay in one HBM buffer, the pool.

`ImageLabelBatches(cache_bytes=...)` keeps whole decoded frames here and csrc/imgload.hip's horizontal pass reads each sample's window
in place (include/mdcv_hip.h, mdcv_imgload_frames_batch); `ConeCropBatches(cache_bytes=...)` keeps whole crops, and the pool is the `src`
of mdcv_kptload_batch.  DESIGN §16.2 has the layout, the admission rule and the stream ordering.

Admission never depends on the order in which samples are drawn: `admit` walks the unique paths in the order given (the CSV's), reserves
3 * w * h bytes rounded up to 256 for each, skips a file that no longer fits and goes on with the next.  Nothing is evicted.

The host half (this module without `ensure_pool`) needs no GPU: `lookup` is where the decode-once rule lives, one lock per file.
"""
import threading

import numpy as np

ALIGN = 256
NEW, DECODED, STAGED, FILLED, REJECTED = range(5)      # an entry's life; REJECTED: its decode did not have the planned size


def _round(n, a=ALIGN):
    return (n + a - 1) // a * a


def admit(paths, sizes, budget, limit=None):
    """-> ({path: (offset, nbytes, (w, h))}, bytes_reserved).  `paths` may repeat (one entry per sample); the first size of a path counts.
    `limit`: no slot ends past this byte (an `int` offset in a descriptor)."""
    budget = int(budget)
    if budget < 0:
        raise ValueError(f"cache_bytes must be None or a byte count >= 0, got {budget}")
    room = budget if limit is None else min(budget, int(limit))
    slots, top = {}, 0
    seen = set()
    for path, (w, h) in zip(paths, sizes):
        if path in seen:
            continue
        seen.add(path)
        n = 3 * int(w) * int(h)
        if n <= 0 or top + _round(n) > room:
            continue
        slots[path] = (top, n, (int(w), int(h)))
        top += _round(n)
    return slots, top


class Entry:
    def __init__(self, path, offset, nbytes, size):
        self.path, self.offset, self.nbytes, self.size = path, offset, nbytes, size
        self.lock, self.state, self.frame = threading.Lock(), NEW, None


class FrameCache:
    """The admission plan, one `Entry` per admitted file, the pool and the counters.  `tail`: bytes kept behind the slots for data that
    changes per batch (the key-point loader's staged crops); the image loader keeps none."""

    def __init__(self, paths, sizes, budget, limit=None, tail=0):
        self.budget, self.tail = int(budget), int(tail)
        slots, self.bytes_reserved = admit(paths, sizes, budget, limit)
        self.entries = {p: Entry(p, o, n, s) for p, (o, n, s) in slots.items()}
        self.pool, self.last_fill = None, None
        self._lock = threading.Lock()
        self._count = dict(hits=0, fills=0, not_admitted=0, size_mismatch=0)

    def _add(self, key):
        with self._lock:
            self._count[key] += 1

    def lookup(self, path, decode):
        """One sample of `path` -> (entry, None): read the pool; or (None, frame): the sample is staged from `frame`.
        `decode(path)` -> (H, W, >= 3) uint8; it runs at most once per admitted file whatever the number of threads asking."""
        ent = self.entries.get(path)
        if ent is None:
            self._add("not_admitted")
            return None, decode(path)
        with ent.lock:
            if ent.state == NEW:
                frame = decode(path)
                if (frame.shape[1], frame.shape[0]) != ent.size:
                    ent.state = REJECTED
                    self._add("size_mismatch")
                    return None, frame
                ent.frame = np.ascontiguousarray(frame[:, :, :3])
                ent.state = DECODED
                self._add("fills")
                return ent, None
            if ent.state != REJECTED:
                self._add("hits")
                return ent, None
        self._add("size_mismatch")
        return None, decode(path)

    def take_fills(self, entries):
        """The entries of one batch whose frame still has to go up, each once; call from one thread at a time (the stager)."""
        out = []
        for ent in entries:
            if ent is not None and ent.state == DECODED:
                ent.state = STAGED
                out.append(ent)
        return out

    def filled(self, entries, event):
        """The copies into the slots of `entries` are enqueued; `event` is recorded behind them on their stream."""
        for ent in entries:
            ent.state, ent.frame = FILLED, None
        if entries:
            self.last_fill = event

    def restart(self):
        """A new epoch: frames staged by an epoch that was abandoned before their batch was enqueued go up with their next batch."""
        for ent in self.entries.values():
            if ent.state == STAGED:
                ent.state = DECODED

    def ensure_pool(self, device):
        import torch
        n = min(self.budget, self.bytes_reserved) + self.tail
        if self.pool is None and n > 0:
            self.pool = torch.empty(n, dtype=torch.uint8, device=device)
        return self.pool

    @property
    def pool_bytes(self):
        return 0 if self.pool is None else int(self.pool.numel())

    def stats(self):
        with self._lock:
            c = dict(self._count)
        return dict(hits=c["hits"], fills=c["fills"], misses=dict(not_admitted=c["not_admitted"], size_mismatch=c["size_mismatch"]),
                    bytes_reserved=self.bytes_reserved, pool_bytes=self.pool_bytes)

    def close(self):
        """Free the pool; a loader iterated again decodes again."""
        self.pool, self.last_fill = None, None
        for ent in self.entries.values():
            ent.state, ent.frame = NEW, None
