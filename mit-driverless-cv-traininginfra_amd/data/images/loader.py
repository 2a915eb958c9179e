"""`ImageLabelBatches`: the loader over the CSV data set, on the staged-batch pipeline of mdcv/data/staging.py."""
import random
import warnings

import numpy as np
import torch

from ... import _lib
from .. import framecache
from ..staging import StagedBatches, copy_fills_device, copy_fills_host, fills_behind
from .augment import Augmentation, ImageFx, draw_augmentation, draw_imgfx, inverse_affine_matrix
from .batch import STAGED, launch_batch, pack_batch, pack_layout
from .geometry import crop_window, frame_reference, n_patches, sample_geometry
from .labels import read_label_csv, sample_labels


class ImageLabelBatches(StagedBatches):
    """Iterable of `(uris, imgs [B,C,H,W] fp32, targets [B,T,5] fp32)` on the device, C = 1 when `bw` else 3: the batches that
    `DataLoader(ImageLabelDataset(path, dataset_path, width, height, ..., num_images, bw, lr_flip, ts), batch_size, shuffle)` yields.

    `decode(path)` -> a PIL image or an (H, W, 3) uint8 array (default: `PIL.Image.open(path).convert('RGB')`), run on `num_workers`
    threads.  `augment_hsv` / `augment_affine` / `data_aug` (both) turn on the reference's ColorJitter / affine augmentation, `blur` /
    `noise` / `contrast` / `sharpen` its four imgaug options (not with `bw`: the reference then hands a 2-D array to
    `Image.fromarray(..., 'RGB')`; ValueError); `salt` is accepted and ignored with a warning, as the reference stores it and never
    reads it.  `draws(epoch, index)` -> (patch_index, flip), (patch_index, flip, aug) or (patch_index, flip, aug, fx) overrides the
    random draws (tests); `aug` is None, an `Augmentation`, or a dict with `jitter` and / or `affine` in `Augmentation`'s form; `fx` is
    None, an `ImageFx`, or a dict with `blur`, `noise`, `contrast`, `sharpen` in `ImageFx`'s form; what is left out stays as drawn.
    `subset_seed` seeds the `random.sample` of `num_images`; its default 0 is the `random.seed(0)` that CVC-YOLOv3/train.py:40 runs
    before it builds its loaders, so the training loader's subset is the one train.py draws.  `debug_mode` forces patch 0 as the
    reference does (the patch draw still happens first, so the flip draw is unchanged).  With `prefetch`, the next batches are decoded
    and staged while one is consumed.

    `cache_bytes`: None, or the HBM budget of a device-resident frame cache (mdcv/data/framecache.py).  Files are admitted
    in CSV order by their CSV sizes until the budget is used; an admitted file is decoded once in the loader's lifetime, its whole frame
    stays on the device, and from then on its samples stage no pixels: the resize reads their windows in place.  The batches are the
    same bytes with and without it.  `cache_stats()` counts what happened; `close()` frees the pool.
    """

    def __init__(self, path, dataset_path, width, height, num_images=-1, bw=False, lr_flip=False, ts=True, batch_size=1, shuffle=True,
                 num_workers=None, seed=0, device=None, decode=None, ud_flip=False, subset_seed=0, draws=None, prefetch=True, debug_mode=False,
                 augment_hsv=False, augment_affine=False, data_aug=False, cache_bytes=None, **options):
        self.blur, self.noise, self.contrast, self.sharpen = (bool(options.pop(k, False)) for k in ("blur", "noise", "contrast", "sharpen"))
        self.salt = options.pop("salt", False)                   # accepted and ignored: the reference stores it and never reads it
        if self.salt:
            warnings.warn("ImageLabelBatches: salt is ignored, as in the reference (ImageLabelDataset stores it and never reads it)")
        self._fx_on = self.blur or self.noise or self.contrast or self.sharpen
        if self._fx_on and bw:
            raise ValueError("ImageLabelBatches: blur / noise / contrast / sharpen cannot be combined with bw (the reference builds an "
                             "'RGB' image from the 2-D grayscale array there, which has no defined meaning)")
        for k in ("vis_batch", "upload_dataset", "n_cpu"):
            options.pop(k, None)
        if options:
            raise TypeError(f"ImageLabelBatches: unknown arguments {sorted(options)}")
        self.width, self.height, self.bw, self.lr_flip, self.ts = int(width), int(height), bool(bw), bool(lr_flip), bool(ts)
        self.ud_flip = ud_flip                                   # accepted and ignored, as in the reference
        self.augment_hsv, self.augment_affine, self.data_aug = bool(augment_hsv), bool(augment_affine), bool(data_aug)
        self.debug_mode = bool(debug_mode)
        self.batch_size, self.shuffle, self.seed, self.draws = int(batch_size), bool(shuffle), int(seed), draws
        self.img_files, self.labels, self.scales, self.sizes = [], [], [], []
        for file, w, h, scale, boxes in read_label_csv(path, dataset_path):
            n = n_patches(w, h, scale, self.width, self.height) if self.ts else 1
            self.img_files += [file] * n
            self.labels += [boxes] * n
            self.scales += [scale] * n
            self.sizes += [(w, h)] * n
        if num_images >= 0:
            idx = random.Random(subset_seed).sample(range(len(self.img_files)), k=num_images)
            if len(idx) > 1:                                     # the reference keeps everything for k <= 1
                for name in ("img_files", "labels", "scales", "sizes"):
                    v = getattr(self, name)
                    setattr(self, name, [v[i] for i in idx])
        self.num_targets_per_image = max((len(l) for l in self.labels), default=0)
        self.dataset = range(len(self.img_files))               # len(loader.dataset), as train.py prints it
        self.epoch = 0
        self._init_staging(num_workers, decode, prefetch, device,
                           None if cache_bytes is None else framecache.FrameCache(self.img_files, self.sizes, cache_bytes))

    def __len__(self):
        return (len(self.img_files) + self.batch_size - 1) // self.batch_size

    @property
    def channels(self):
        return 1 if self.bw else 3

    def order(self, epoch):
        idx = list(range(len(self.img_files)))
        if self.shuffle:
            random.Random(f"{self.seed}/{epoch}/order").shuffle(idx)
        return idx

    def plan(self, index, epoch=0, frame_size=None):
        """Host-only: the draws, geometry, augmentation (`.aug`: None or an `Augmentation` with its matrix; `.fx`: None or an `ImageFx`)
        and labels of sample `index` in `epoch` (frame_size: the decoded (W, H); default the CSV's)."""
        w, h = frame_size if frame_size is not None else self.sizes[index]
        rng = random.Random(f"{self.seed}/{epoch}/{index}")
        patch = rng.randint(0, n_patches(w, h, self.scales[index], self.width, self.height) - 1) if self.ts else 0
        if self.debug_mode:
            patch = 0
        boxed = len(self.labels[index]) > 0                          # raw-empty samples return before the augmentation and the flip
        aug = None
        if boxed and (self.augment_hsv or self.augment_affine or self.data_aug):
            aug = draw_augmentation(rng, self.augment_hsv or self.data_aug, self.augment_affine or self.data_aug)
        flip = bool(self.lr_flip and boxed and rng.random() > 0.5)
        fx = None
        if boxed and self._fx_on:
            fx = draw_imgfx(rng, lambda: random.Random(f"{self.seed}/{epoch}/{index}/imgaug"), self.blur, self.noise, self.contrast, self.sharpen)
        if self.draws is not None:
            d = self.draws(epoch, index)
            patch, flip = d[0], bool(d[1]) and boxed
            if len(d) > 2:
                aug = d[2] if boxed else None
                if isinstance(aug, dict):
                    aug = Augmentation(aug.get("jitter"), aug.get("affine"))
            if len(d) > 3:
                fx = d[3] if boxed else None
                if isinstance(fx, dict):
                    fx = ImageFx(fx.get("blur"), fx.get("noise"), fx.get("contrast"), fx.get("sharpen"))
                if fx and self.bw:
                    raise ValueError("blur / noise / contrast / sharpen cannot be combined with bw")
        if aug is not None and aug.affine is not None:
            aug.matrix = inverse_affine_matrix(self.width, self.height, *aug.affine)
        g = sample_geometry(w, h, self.width, self.height, self.ts, self.scales[index] if self.ts else 1.0, patch, flip)
        g.index, g.uri = index, self.img_files[index]
        g.aug = aug if aug else None
        g.fx = fx if fx else None
        g.labels = sample_labels(self.labels[index], g, self.num_targets_per_image, g.aug)
        return g

    # -- host half: decode, plan, crop, stage
    def _decode(self, path):
        img = self.decode(path)
        frame = img if isinstance(img, np.ndarray) else np.asarray(img, dtype=np.uint8)
        if frame.ndim != 3 or frame.shape[2] < 3 or frame.dtype != np.uint8:
            raise ValueError(f"{path}: decode must give an (H, W, 3) uint8 RGB frame, got {frame.shape} {frame.dtype}")
        return frame

    def _sample(self, epoch, index):
        """-> (geometry, window bytes or None, cache entry or None): a sample of a cached frame has no window, only its entry"""
        if self._cache is not None:
            ent, frame = self._cache.lookup(self.img_files[index], self._decode)
            if ent is not None:
                return self.plan(index, epoch, ent.size), None, ent
        else:
            frame = self._decode(self.img_files[index])
        g = self.plan(index, epoch, (frame.shape[1], frame.shape[0]))
        return g, crop_window(frame, g), None

    def _stage(self, epoch, bi, slot):
        order = self._orders[epoch]
        got = self._map(lambda i: self._sample(epoch, i), order[bi * self.batch_size:(bi + 1) * self.batch_size])
        geoms, windows, ents = [g for g, _, _ in got], [w for _, w, _ in got], [e for _, _, e in got]
        frefs, fills = None, []
        if any(e is not None for e in ents):                     # a batch with no cached sample is staged and launched as without a cache
            frefs = [STAGED if e is None else frame_reference(g, e.offset) for g, e in zip(geoms, ents)]
            fills = self._cache.take_fills(ents)
        p = pack_layout(geoms, [0 if w is None else w.nbytes for w in windows], self.num_targets_per_image, frefs)
        p.fills, need = fills_behind(p.nbytes, fills)            # first sight: the whole frames ride behind the batch, one copy each
        host = slot.buffer(need).numpy()
        pack_batch(host, p, geoms, windows, [g.labels for g in geoms], frefs)
        copy_fills_host(host, p.fills)
        return [g.uri for g in geoms], p, slot

    # -- device half: one H2D copy and the kernel pair on the side stream
    def _enqueue(self, staged):
        uris, p, slot = staged
        dev = self.device
        with torch.cuda.device(dev), torch.cuda.stream(self._stream):
            dbuf = torch.empty(p.nbytes, dtype=torch.uint8, device=dev)
            dbuf.copy_(slot.pinned[:p.nbytes], non_blocking=True)
            pool = self._cache.pool if p.fref else None
            if p.fref:
                copy_fills_device(pool, slot.pinned, p.fills)
            self._copied(slot, p.fills)
            imgs = launch_batch(dbuf, slot.pinned.numpy(), p, self.channels, self.height, self.width, self._stream, pool)
            tg = dbuf[p.lab_off:p.lab_off + p.B * p.T * 20].view(torch.float32).view(p.B, p.T, 5).clone()
            return uris, imgs, tg, self._ready()

    def __iter__(self):
        _lib.require_gpu()
        epoch = self.epoch
        self.epoch += 1
        self._orders = {epoch: self.order(epoch)}
        yield from self._batches(len(self), lambda bi, slot: self._stage(epoch, bi, slot))
