"""The lagging step log of the native training loops (mdcv/yolo/train.py, mdcv/rektnet/train.py).

The reference's loops read every loss of every step back with `.item()` (CVC-YOLOv3/train.py:63,75,85-89: sixteen blocking reads per step;
RektNet/train_eval.py:74: three) to print a line and to add to the epoch's sums.  Here a step ends with ONE launch (`mdcv_train_log_step`,
csrc/train_log.hip) that writes the step's row -- its losses and its count of labelled targets -- into a device ring and adds them to fp64
sums on the device, in the order and with the roundings of the loop's Python floats.  The row follows to a pinned host ring with a
non-blocking copy and an event; the host formats a step's line when its row has LANDED, which it finds out with `event.query()`.  Lines
therefore come out a few steps late, complete and in step order, and the host waits for the GPU only when the ring is full and once at the
end of the epoch (`StepLog.host_waits` counts both).

    log = StepLog(7, on_row=lambda i, row, meta: print(format(i, row)))
    for batch in batches:
        log.drain()                      # hand out what has landed
        ... forward / backward / optimizer.step() ...
        log.record(losses, targets)
    log.drain(block=True)                # the epoch's one wait
    sums = log.sums()

`RowRing` is the slot and order logic alone (no GPU: tests drive it with a fake event); `prefetch` moves host batches to the device one
batch ahead on a copy stream.
"""
import ctypes

import torch

from . import _lib

ROW = 12                                   # MDCV_TRAIN_LOG_ROW
MAX_LOSSES = 8                             # MDCV_TRAIN_LOG_MAX_LOSSES


class RowRing:
    """Which slot step i writes, and when its row may be handed out.  Step i uses slot i % ring; `head` is the oldest step not yet handed
    out, `tail` the next step to record, 0 <= tail - head <= ring.  Events need `query()` and `synchronize()`; the events of one ring are
    recorded on one stream, so they land in step order -- and rows are handed out in step order whatever `query()` says about later ones.

    `on_row(step, row, meta)`: row = `read(slot)` at hand-out time, meta = what `push` was given."""

    def __init__(self, ring, read, on_row):
        if ring < 1:
            raise ValueError("RowRing: ring must be >= 1")
        self.ring, self.read, self.on_row = int(ring), read, on_row
        self.head = self.tail = 0
        self.events, self.meta = [None] * self.ring, [None] * self.ring
        self.host_waits = 0

    def _hand_out(self):
        s = self.head % self.ring
        meta, self.meta[s], self.events[s] = self.meta[s], None, None
        self.head += 1                                   # (before the callback: a formatter that raises does not get its row twice)
        self.on_row(self.head - 1, self.read(s), meta)

    def next_slot(self):
        """the slot of the step about to be recorded.  Ring full: waits for the oldest row (a host wait, counted) and hands it out."""
        if self.tail - self.head == self.ring:
            ev = self.events[self.head % self.ring]
            if not ev.query():
                ev.synchronize()
                self.host_waits += 1
            self._hand_out()
        return self.tail % self.ring

    def push(self, event, meta=None):
        """the step's launch and copy are queued into `next_slot()` and `event` is recorded behind them"""
        s = self.tail % self.ring
        assert self.tail - self.head < self.ring and self.events[s] is None
        self.events[s], self.meta[s] = event, meta
        self.tail += 1

    def drain(self, block=False):
        """hands out every landed row, oldest first, and stops at the first that has not landed; block: waits ONCE, for the newest row
        (counted), after which every row has landed"""
        if block and self.tail > self.head:
            ev = self.events[(self.tail - 1) % self.ring]
            ev.synchronize()
            self.host_waits += 1
        n = 0
        while self.head < self.tail and (block or self.events[self.head % self.ring].query()):
            self._hand_out()
            n += 1
        return n


def _source(t, what):
    """a loss source: None, or a one-element fp32 tensor on the device (a view is fine: only its address is kept)"""
    if t is None:
        return None
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.numel() == 1):
        raise ValueError(f"StepLog.record: {what} must be None or a one-element float32 tensor on the GPU")
    return t.detach()


class StepLog:
    """Device ring [ring, ROW] fp32 + pinned host ring + one event per slot + the fp64 sums [n_losses + 1] (module docstring).

    `on_row(step, row, meta)`: row = n_losses + 1 Python floats (the step's fp32 losses and its target count, widened exactly as `.item()`
    widens them).  One StepLog serves one epoch; `reset()` starts the next (sums to 0.0, the count word to 1e-12 as train.py:54).
    `record` and `drain(block=True)` must be called with the same current stream: the stream the steps run on."""

    def __init__(self, n_losses, ring=64, device=None, on_row=None):
        _lib.require_gpu()
        if not 1 <= n_losses <= MAX_LOSSES:
            raise ValueError(f"StepLog: n_losses must be in 1..{MAX_LOSSES}")
        self.n = int(n_losses)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.on_row = on_row
        self._dev = torch.zeros(int(ring), ROW, dtype=torch.float32, device=self.device)
        self._host = torch.zeros(int(ring), ROW, dtype=torch.float32).pin_memory()
        self._acc = torch.zeros(self.n + 1, dtype=torch.float64, device=self.device)
        self._acc_host = torch.zeros(self.n + 1, dtype=torch.float64).pin_memory()
        self._acc_init = torch.tensor([0.0] * self.n + [1e-12], dtype=torch.float64).pin_memory()
        self._free_events = [torch.cuda.Event() for _ in range(int(ring))]
        self._ptrs = (ctypes.c_void_p * MAX_LOSSES)()
        self._ring = RowRing(ring, self._read, self._emit)
        self._end, self._end_waits = torch.cuda.Event(), 0
        self._sums = None
        self.reset()

    @property
    def host_waits(self):
        """times the host waited for the GPU: ring-full waits in `record` + the end-of-epoch waits of `drain(block=True)`"""
        return self._ring.host_waits + self._end_waits

    @property
    def steps(self):
        return self._ring.tail

    def reset(self):
        """the next epoch: steps count from 0 again, the sums start over (`host_waits` keeps counting)"""
        if self._ring.tail != self._ring.head:
            raise RuntimeError("StepLog.reset: rows are still in flight; drain(block=True) first")
        self._ring.head = self._ring.tail = 0
        self._acc.copy_(self._acc_init, non_blocking=True)       # stream-ordered in front of the next epoch's first launch
        self._sums = None

    def _read(self, slot):
        return self._host[slot, :self.n + 1].tolist()

    def _emit(self, step, row, held):
        if self.on_row is not None:
            self.on_row(step, row, held[0])                      # held = (meta, the sources, the targets) of `record`

    def record(self, losses, targets=None, meta=None):
        """Queues, on the current stream: the bookkeeping launch of one step into the next slot, the row's copy to the pinned ring, the
        slot's event.  losses: n_losses sources (None = 0.0); targets: None or [B,T,5] fp32 on the device."""
        if len(losses) != self.n:
            raise ValueError(f"StepLog.record: {len(losses)} losses, the log was built for {self.n}")
        srcs = [_source(t, f"loss {j}") for j, t in enumerate(losses)]
        B = T = 0
        tp = None
        if targets is not None:
            if not (targets.is_cuda and targets.dtype == torch.float32 and targets.dim() == 3 and targets.shape[2] == 5):
                raise ValueError("StepLog.record: targets must be a [B,T,5] float32 tensor on the GPU")
            targets = targets.detach().contiguous()
            B, T = int(targets.shape[0]), int(targets.shape[1])
            tp = targets.data_ptr() if B * T else None
        ring = self._ring
        slot = ring.next_slot()
        for j in range(MAX_LOSSES):
            self._ptrs[j] = srcs[j].data_ptr() if j < self.n and srcs[j] is not None else None
        L = _lib.lib()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream()
            L.check(L.train_log_step(ctypes.addressof(self._ptrs), self.n, tp, int(targets is not None), B, T, self._acc.data_ptr(),
                                     self._dev[slot].data_ptr(), stream.cuda_stream), "train_log_step")
            # (on the steps' own stream: a copy stream of its own, fed by an event behind the launch, measured 0.16 ms per YOLOv3 step SLOWER)
            self._host[slot].copy_(self._dev[slot], non_blocking=True)
            ev = self._free_events[slot]
            ev.record(stream)
        self._sums = None
        ring.push(ev, (meta, srcs, targets))                     # (the sources stay referenced until their row has been handed out)

    def drain(self, block=False):
        """Hands every landed row to `on_row`, in step order.  block=True: the epoch's end -- also fetches the sums, and waits once."""
        if block:
            with torch.cuda.device(self.device):
                self._acc_host.copy_(self._acc, non_blocking=True)
                self._end.record()
            self._end.synchronize()                              # behind every row's copy on the same stream: they have all landed
            self._end_waits += 1
            n = self._ring.drain(block=False)
            assert self._ring.head == self._ring.tail
            self._sums = self._acc_host.tolist()
            return n
        return self._ring.drain(block=False)

    def sums(self):
        """[sum of loss_0, .., sum of loss_{n-1}, 1e-12 + sum of (count + 1e-12)] as Python floats: the device's fp64 words, read once"""
        if self._sums is None:
            self.drain(block=True)
        return list(self._sums)


def _on_device(item):
    return all(t.is_cuda for t in item if torch.is_tensor(t))


def prefetch(loader, device):
    """Yields the loader's batches with every tensor on `device`.  Batch i+1's `.to(device, non_blocking=True)` is issued on a copy stream
    before batch i is handed over; the consumer's stream waits for a batch's copies when it is handed over, never the host.  (The copies
    overlap compute when the loader's tensors are pinned, as with DataLoader(pin_memory=True).)  Non-tensor members pass through."""
    dev = torch.device(device)
    copy = torch.cuda.Stream(dev)

    def issue(item):
        with torch.cuda.stream(copy):
            moved = tuple(t.to(dev, non_blocking=True) if torch.is_tensor(t) else t for t in item)
            ev = torch.cuda.Event()
            ev.record(copy)
        return moved, ev

    it = iter(loader)
    try:
        nxt = issue(next(it))
    except StopIteration:
        return
    while nxt is not None:
        (moved, ev), nxt = nxt, None
        try:
            nxt = issue(next(it))
        except StopIteration:
            pass
        cons = torch.cuda.current_stream(dev)
        cons.wait_event(ev)
        for t in moved:
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(cons)
        yield moved


def device_batches(loader, device):
    """The loader's batches on the device: as they are when the loader already yields device tensors (ImageLabelBatches, ConeCropBatches,
    SyntheticCones, a list of device batches), through `prefetch` otherwise.  Decided on the first batch."""
    it = iter(loader)
    try:
        first = next(it)
    except StopIteration:
        return

    def chain():
        yield first
        yield from it
    if _on_device(first):
        yield from chain()
    else:
        yield from prefetch(chain(), device)
