"""Mosaic augmentation of detector batches on the device (csrc/mosaic.hip behind include/mdcv_aug.h).

`MosaicBatches(loader)` wraps any iterable of `(uris, imgs [B,C,H,W] fp32, targets [B,T,5] fp32)` device batches -- `ImageLabelBatches`,
`SyntheticCones`, a list -- and yields `(uris, out, targets_out [B,4T,5])`: every image composed from the corners of four images of its
own batch around a drawn centre, the labels shifted, clipped to their quadrant, filtered and packed, in ONE launch per batch on the current
stream.  The draws are host-side integers (8 per image) that reach the device through pinned memory; nothing is read back per batch.
"""
import math
import random

import numpy as np
import torch

from .. import _lib

DESC = 8


def draw_rows(seed, epoch, index, B, H, W, p=1.0, centre=(0.25, 0.75)):
    """The descriptor rows `[apply, xc, yc, s0, s1, s2, s3, 0]` of batch `index` of epoch `epoch`: a pure function of its arguments.  Per
    image, in order, from `random.Random(f"{seed}/{epoch}/{index}/mosaic")`: `apply = random() < p`; three partners `randrange(B)`; the
    sources `[b, p1, p2, p3]` shuffled (so b is always one of them); `xc = randint(ceil(c0 W), floor(c1 W))` clamped to [1, W-1], and `yc`
    likewise.  Every image consumes the same draws whether or not it is applied."""
    rng = random.Random(f"{seed}/{epoch}/{index}/mosaic")
    rows = []
    for b in range(B):
        apply = rng.random() < p
        src = [b, rng.randrange(B), rng.randrange(B), rng.randrange(B)]
        rng.shuffle(src)
        c = []
        for n in (W, H):
            lo = math.ceil(centre[0] * n)
            c.append(min(max(rng.randint(lo, max(lo, math.floor(centre[1] * n))), 1), n - 1))      # an empty range draws its lower end
        rows.append([int(apply), c[0], c[1], *src, 0])
    return rows


class MosaicBatches:
    def __init__(self, loader, p=1.0, seed=0, centre=(0.25, 0.75), min_px=2.0, min_visible=0.25, draws=None):
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"MosaicBatches: p {p} is outside [0, 1]")
        if not (len(centre) == 2 and 0.0 <= centre[0] <= centre[1] <= 1.0):
            raise ValueError(f"MosaicBatches: centre {centre} is not a range inside [0, 1]")
        if not min_px >= 1.0:
            raise ValueError(f"MosaicBatches: min_px {min_px} is below 1 pixel")
        if not 0.0 <= min_visible <= 1.0:
            raise ValueError(f"MosaicBatches: min_visible {min_visible} is outside [0, 1]")
        self.loader, self.p, self.seed, self.centre = loader, float(p), seed, (float(centre[0]), float(centre[1]))
        self.min_px, self.min_visible, self.draws = float(min_px), float(min_visible), draws
        self.active = True
        self.epoch = 0                      # epochs started: the e of the draws
        self._stats = None                  # int32[4] on the device, accumulated by the kernel between two reads
        self._totals = [0, 0, 0, 0]         # what the reads have collected: Python integers, no 2^31
        self._images = self._composed = 0   # host-side counts (they need no read)
        self._seen = dict(kept=0, dropped=0, overflow=0, images=0, composed=0)

    def __len__(self):
        return len(self.loader)

    @property
    def dataset(self):
        return self.loader.dataset

    def close(self):
        close = getattr(self.loader, "close", None)
        if close is not None:
            close()

    def rows(self, epoch, index, B, H, W):
        """the descriptor rows of one batch as an int32 array [B, 8]: `draws(epoch, index, B)` when given, `draw_rows` otherwise"""
        rows = self.draws(epoch, index, B) if self.draws is not None else draw_rows(self.seed, epoch, index, B, H, W, self.p, self.centre)
        rows = np.asarray(rows, dtype=np.int32)
        if rows.shape != (B, DESC):
            raise ValueError(f"MosaicBatches: {B} rows of {DESC} integers expected, got an array of shape {rows.shape}")
        return rows

    def compose(self, rows, imgs, targets):
        """one batch through the kernel, on the current stream -> (out, targets_out [B, 4T, 5])"""
        _lib.require_gpu(imgs)
        _lib.require_gpu(targets)
        if imgs.dtype != torch.float32 or targets.dtype != torch.float32 or imgs.dim() != 4 or targets.dim() != 3 or targets.shape[2] != 5 \
                or targets.shape[0] != imgs.shape[0]:
            raise ValueError(f"MosaicBatches: imgs [B,C,H,W] and targets [B,T,5] in float32 expected, got {tuple(imgs.shape)} {imgs.dtype} "
                             f"and {tuple(targets.shape)} {targets.dtype}")
        A = _lib.aug_lib()
        imgs, targets = imgs.contiguous(), targets.contiguous()
        B, C, H, W = imgs.shape
        T = targets.shape[1]
        dev = imgs.device
        with torch.cuda.device(dev):
            if self._stats is None or self._stats.device != dev:
                self._stats = torch.zeros(4, dtype=torch.int32, device=dev)
            # a fresh pinned block per batch: the caching host allocator keeps it alive until the copy below has run
            host = torch.empty((B, DESC), dtype=torch.int32, pin_memory=True)
            host.numpy()[...] = rows
            desc = host.to(dev, non_blocking=True)
            out = torch.empty_like(imgs)
            tout = torch.empty((B, 4 * T, 5), dtype=torch.float32, device=dev)
            A.check(A.mosaic_batch(host.data_ptr(), desc.data_ptr(), B, C, H, W, imgs.data_ptr(), out.data_ptr(), targets.data_ptr(), T,
                                   tout.data_ptr(), 4 * T, self.min_px, self.min_visible, self._stats.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream), "mosaic_batch")
        self._images += B
        self._composed += int((rows[:, 0] == 1).sum())
        return out, tout

    def __iter__(self):
        if not self.active:
            yield from self.loader
            return
        self.epoch += 1
        e = self.epoch
        for i, (uris, imgs, targets) in enumerate(self.loader):
            B, _, H, W = imgs.shape
            out, tout = self.compose(self.rows(e, i, B, H, W), imgs, targets)
            yield uris, out, tout

    def stats(self):
        """-> {kept, dropped, overflow, errors, images, composed}, totals since construction: label rows kept, candidates the rule dropped,
        kept rows lost beyond 4T (never, by construction), the kernel's error bits; images seen and images composed.  ONE host read; raises
        when an error bit is set (a descriptor that was good on the host reached the kernel bad).  The device counters are int32: each read
        adds them to Python integers and zeroes them (on the current stream, in order with the launches), so they only have to hold what
        accumulates between two reads -- the loops read once per epoch."""
        if self._stats is not None:
            with torch.cuda.device(self._stats.device):
                got = self._stats.cpu().tolist()
                self._stats.zero_()
            self._totals = [a + b for a, b in zip(self._totals[:3], got[:3])] + [self._totals[3] | got[3]]
        s = self._totals
        if s[3]:
            raise _lib.MdcvError(f"MosaicBatches: the kernel rejected a device descriptor (error bits {s[3]:#x}); those images passed through")
        return dict(kept=s[0], dropped=s[1], overflow=s[2], errors=s[3], images=self._images, composed=self._composed)

    def summary_line(self, label_prefix, epoch):
        """the training loop's one line per epoch (one host read): the counts since the line before"""
        s = self.stats()
        d = {k: s[k] - self._seen[k] for k in self._seen}
        self._seen = {k: s[k] for k in self._seen}
        if d["images"] == 0:
            return f"{label_prefix} Epoch: {epoch}, mosaic off: batches handed through"
        return (f"{label_prefix} Epoch: {epoch}, mosaic: {d['composed']} of {d['images']} images composed, label rows kept {d['kept']}, "
                f"dropped {d['dropped']}, overflow {d['overflow']}")
