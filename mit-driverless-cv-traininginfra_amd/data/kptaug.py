"""Augmentation of key-point batches on the device (csrc/kptaug.hip behind include/mdcv_kptaug.h).

`KeypointAugBatches(loader)` wraps any iterable of `(imgs [B,C,S,S], hm [B,7,S,S], pts [B,7,2], names, sizes)` device batches --
`ConeCropBatches`, `SyntheticConeCrops`, a list -- and yields the same 5-tuple: every crop rotated, scaled, shifted and perhaps mirrored
about its centre (bilinear, edge replicate), its channels scaled and offset, its seven key points sent through the same map (left and right
exchanged under a mirror) and its heat-maps regenerated from the new points, in ONE launch per batch on the current stream.  A draw that
would push a key point out of the crop is rejected ON THE DEVICE (the image passes through as it is), so the host never needs the points.
The draws are host-side numbers (24 words per image) that reach the device through pinned memory; nothing is read back per batch.
"""
import math
import random

import numpy as np
import torch

from .. import _lib

DESC = 24
APPLY, SWAP = 1, 2
PERM = (0, 2, 1, 4, 3, 6, 5)            # the partner of each key point under a left/right mirror


def affine_maps(S, degrees=0.0, scale=1.0, tx=0.0, ty=0.0, flip=False):
    """-> (F, I), float64 [2,3] each, in pixel-index coordinates: F = T(c + t) R(degrees) Scale(scale) Flip T(-c) with c = (S - 1) / 2
    sends a source point to its output point, and I is F's inverse written out (the transposed rotation, 1 / scale, the mirror again),
    not computed from F: I sends an output pixel index to its source pixel index."""
    c = (S - 1) / 2.0
    th = math.radians(degrees)
    co, si, fl = math.cos(th), math.sin(th), (-1.0 if flip else 1.0)
    a = np.array([[co * scale * fl, -si * scale], [si * scale * fl, co * scale]])
    ai = np.array([[fl * co / scale, fl * si / scale], [-si / scale, co / scale]])
    F = np.empty((2, 3))
    I = np.empty((2, 3))
    F[:, :2], I[:, :2] = a, ai
    F[:, 2] = np.array([c + tx, c + ty]) - a @ np.array([c, c])
    I[:, 2] = np.array([c, c]) - ai @ np.array([c + tx, c + ty])
    return F, I


def descriptor(S, apply=True, degrees=0.0, scale=1.0, tx=0.0, ty=0.0, flip=False, gain=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
    """one descriptor row, int32 [24] (include/mdcv_kptaug.h): every float64 entry rounded once to fp32 and carried as its bits"""
    F, I = affine_maps(S, degrees, scale, tx, ty, flip)
    row = np.zeros(DESC, np.int32)
    row[0] = (APPLY if apply else 0) | (SWAP if flip else 0)
    row[1:19] = np.concatenate([I.ravel(), F.ravel(), np.asarray(gain, np.float64), np.asarray(bias, np.float64)]).astype(np.float32).view(np.int32)
    return row


def draw_params(seed, epoch, index, B, S, p=1.0, degrees=15.0, scale=(0.85, 1.15), translate=0.08, flip=0.5, brightness=0.2, contrast=0.2,
                tint=0.05):
    """The drawn parameters of batch `index` of epoch `epoch`, one dict of `descriptor` keywords per image: a pure function of its
    arguments.  Per image, in order, from `random.Random(f"{seed}/{epoch}/{index}/kptaug")`, eleven draws: `apply = random() < p`; the
    angle `uniform(-degrees, degrees)`; the scale `uniform(*scale)`; `tx`, `ty = uniform(-translate, translate) * S`; `flip = random() <
    flip`; brightness `uniform(1 - brightness, 1 + brightness)`, contrast likewise, three tints likewise; `gain_c = contrast * brightness
    * tint_c`, `bias_c = 0.5 * (1 - contrast)`.  Every image consumes the same draws whether or not it is applied."""
    rng = random.Random(f"{seed}/{epoch}/{index}/kptaug")
    out = []
    for _ in range(B):
        apply = rng.random() < p
        deg = rng.uniform(-degrees, degrees)
        sc = rng.uniform(scale[0], scale[1])
        tx, ty = rng.uniform(-translate, translate) * S, rng.uniform(-translate, translate) * S
        fl = rng.random() < flip
        br = rng.uniform(1.0 - brightness, 1.0 + brightness)
        ct = rng.uniform(1.0 - contrast, 1.0 + contrast)
        tints = [rng.uniform(1.0 - tint, 1.0 + tint) for _ in range(3)]
        out.append(dict(apply=apply, degrees=deg, scale=sc, tx=tx, ty=ty, flip=fl, gain=tuple(ct * br * t for t in tints),
                        bias=(0.5 * (1.0 - ct),) * 3))
    return out


def draw_rows(seed, epoch, index, B, S, p=1.0, degrees=15.0, scale=(0.85, 1.15), translate=0.08, flip=0.5, brightness=0.2, contrast=0.2,
              tint=0.05):
    """the descriptor rows of `draw_params`, int32 [B, 24].  `p` decides bit 0 of word 0 and nothing else: a row that is not applied
    carries the maps and gains it drew all the same."""
    return np.stack([descriptor(S, **kw) for kw in draw_params(seed, epoch, index, B, S, p, degrees, scale, translate, flip, brightness,
                                                               contrast, tint)])


class KeypointAugBatches:
    def __init__(self, loader, p=1.0, seed=0, degrees=15.0, scale=(0.85, 1.15), translate=0.08, flip=0.5, brightness=0.2, contrast=0.2,
                 tint=0.05, draws=None):
        if not 0.0 <= p <= 1.0 or not 0.0 <= flip <= 1.0:
            raise ValueError(f"KeypointAugBatches: p {p} or flip {flip} is outside [0, 1]")
        if not (len(scale) == 2 and 0.0 < scale[0] <= scale[1]):
            raise ValueError(f"KeypointAugBatches: scale {scale} is not a range of positive factors")
        if not (0.0 <= degrees <= 180.0 and 0.0 <= translate <= 1.0):
            raise ValueError(f"KeypointAugBatches: degrees {degrees} is outside [0, 180] or translate {translate} outside [0, 1]")
        if not (0.0 <= brightness < 1.0 and 0.0 <= contrast < 1.0 and 0.0 <= tint < 1.0):
            raise ValueError(f"KeypointAugBatches: brightness {brightness}, contrast {contrast} and tint {tint} must lie in [0, 1)")
        self.loader, self.p, self.seed, self.draws = loader, float(p), seed, draws
        self.kw = dict(degrees=float(degrees), scale=(float(scale[0]), float(scale[1])), translate=float(translate), flip=float(flip),
                       brightness=float(brightness), contrast=float(contrast), tint=float(tint))
        self.active = True
        self.epoch = 0                      # epochs started: the e of the draws
        self._stats = None                  # int32[4] on the device, accumulated by the kernel between two reads
        self._totals = [0, 0, 0, 0]         # what the reads have collected: Python integers, no 2^31
        self._images = 0                    # host-side count (it needs no read)
        self._seen = dict(augmented=0, rejected=0, passed=0, images=0)

    def __len__(self):
        return len(self.loader)

    @property
    def dataset(self):
        return self.loader.dataset

    def close(self):
        close = getattr(self.loader, "close", None)
        if close is not None:
            close()

    def rows(self, epoch, index, B, S):
        """the descriptor rows of one batch as an int32 array [B, 24]: `draws(epoch, index, B)` when given, `draw_rows` otherwise"""
        rows = self.draws(epoch, index, B) if self.draws is not None else draw_rows(self.seed, epoch, index, B, S, self.p, **self.kw)
        rows = np.asarray(rows, dtype=np.int32)
        if rows.shape != (B, DESC):
            raise ValueError(f"KeypointAugBatches: {B} rows of {DESC} integers expected, got an array of shape {rows.shape}")
        return rows

    def augment(self, rows, imgs, hm, pts):
        """one batch through the kernel, on the current stream -> (imgs_out, hm_out, pts_out)"""
        for t in (imgs, hm, pts):
            _lib.require_gpu(t)
        if any(t.dtype != torch.float32 for t in (imgs, hm, pts)) or imgs.dim() != 4 or imgs.shape[2] != imgs.shape[3] \
                or tuple(hm.shape) != (imgs.shape[0], 7, imgs.shape[2], imgs.shape[3]) or tuple(pts.shape) != (imgs.shape[0], 7, 2):
            raise ValueError(f"KeypointAugBatches: imgs [B,C,S,S], hm [B,7,S,S] and pts [B,7,2] in float32 expected, got "
                             f"{tuple(imgs.shape)} {imgs.dtype}, {tuple(hm.shape)} {hm.dtype} and {tuple(pts.shape)} {pts.dtype}")
        A = _lib.kptaug_lib()
        imgs, hm, pts = imgs.contiguous(), hm.contiguous(), pts.contiguous()
        B, C, S, _ = imgs.shape
        dev = imgs.device
        with torch.cuda.device(dev):
            if self._stats is None or self._stats.device != dev:
                self._stats = torch.zeros(4, dtype=torch.int32, device=dev)
            # a fresh pinned block per batch: the caching host allocator keeps it alive until the copy below has run
            host = torch.empty((B, DESC), dtype=torch.int32, pin_memory=True)
            host.numpy()[...] = rows
            desc = host.to(dev, non_blocking=True)
            imgs_out, hm_out, pts_out = torch.empty_like(imgs), torch.empty_like(hm), torch.empty_like(pts)
            A.check(A.kptaug_batch(host.data_ptr(), desc.data_ptr(), B, C, S, 7, imgs.data_ptr(), hm.data_ptr(), pts.data_ptr(),
                                   imgs_out.data_ptr(), hm_out.data_ptr(), pts_out.data_ptr(), self._stats.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream), "kptaug_batch")
        self._images += B
        return imgs_out, hm_out, pts_out

    def __iter__(self):
        if not self.active:
            yield from self.loader
            return
        self.epoch += 1
        e = self.epoch
        for i, (imgs, hm, pts, names, sizes) in enumerate(self.loader):
            out = self.augment(self.rows(e, i, imgs.shape[0], imgs.shape[-1]), imgs, hm, pts)
            yield (*out, names, sizes)

    def stats(self):
        """-> {augmented, rejected, passed, errors, images}, totals since construction: images augmented, images whose draw the bounds
        rule rejected (a key point would have left the crop), images passed through by their descriptor, the kernel's error bits; images
        seen.  ONE host read; raises when an error bit is set (a descriptor that was good on the host reached the kernel bad).  The
        device counters are int32: each read adds them to Python integers and zeroes them (on the current stream, in order with the
        launches), so they only have to hold what accumulates between two reads -- the loop reads once per epoch."""
        if self._stats is not None:
            with torch.cuda.device(self._stats.device):
                got = self._stats.cpu().tolist()
                self._stats.zero_()
            self._totals = [a + b for a, b in zip(self._totals[:3], got[:3])] + [self._totals[3] | got[3]]
        s = self._totals
        if s[3]:
            raise _lib.MdcvError(f"KeypointAugBatches: the kernel rejected a device descriptor (error bits {s[3]:#x}); those images passed through")
        return dict(augmented=s[0], rejected=s[1], passed=s[2], errors=s[3], images=self._images)

    def summary_line(self, label_prefix, epoch):
        """the training loop's one line per epoch (one host read): the counts since the line before"""
        s = self.stats()
        d = {k: s[k] - self._seen[k] for k in self._seen}
        self._seen = {k: s[k] for k in self._seen}
        if d["images"] == 0:
            return f"{label_prefix} Epoch: {epoch}, key-point augmentation off: batches handed through"
        return (f"{label_prefix} Epoch: {epoch}, key-point augmentation: {d['augmented']} of {d['images']} images augmented, "
                f"rejected {d['rejected']}, passed through {d['passed']}")
