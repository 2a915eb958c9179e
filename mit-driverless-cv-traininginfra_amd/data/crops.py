"""Real key-point batches: `ConeCropBatches` stands where `DataLoader(ConeDataset(...), batch_size, shuffle=False, num_workers=0)` stands in
RektNet/train_eval.py:255-258, and `load_train_csv_dataset` where RektNet/utils.py:152-235 stands (which needs OpenCV and google.cloud).

The host decodes the crop files (Pillow, on a thread pool) and computes the key points; everything from the decoded uint8 crop to the
`[B,3,S,S]` image and the `[B,7,S,S]` heat-maps runs in csrc/kptload.hip, one launch per batch.  What the reference computes:

* image (dataset.py:35-38,54; utils.py:73-76): `cv2.resize(cv2.imread(path), (S, S))` on the 8-bit image, then `transpose / 255.0` in
  float64 and one rounding to float32.  cv2.imread delivers B, G, R and the reference never swaps, so the planes come out B, G, R.
* heat-maps (utils.py:83-96 `prep_label`): a float64 one-hot at `(int(y), int(x))` of the ORIGINAL crop, `cv2.resize` to S x S, a 5x5
  `cv2.GaussianBlur(sigma=0)`, divided by its sum.  A down-scaled one-hot that no tap reads sums to 0: the reference prints a warning
  and divides 0 / 0; its all-NaN map is kept.  The loader finds such labels on the host from the tap positions (`_read_mask`, a third
  statement of which samples INTER_LINEAR reads, checked against the oracle), prints the warning and collects the name in `.incorrect_labels`.
* points (utils.py:98-111, dataset.py:41-43): `math.ceil(int(pt) * scale) / S` in Python doubles, `scale = S / orig`, then float32; computed
  here on the host and shipped with the pixels in the same pinned buffer and the same copy.
* `hm_tmp[int(y), int(x)] = 1.0` raises IndexError for a label beyond the crop; so does this loader, naming the image, before anything
  is enqueued.  The reference lets a NEGATIVE index wrap round to the other edge silently; here it raises too.

Parity with cv2 itself is unpinned (OpenCV is not available to this project): the two cv2 calls are the restatements of DESIGN §10 and §11,
shared with `mdcv_crop_resize_u8` and `SyntheticConeCrops`.
"""
import hashlib
import math
import os
from functools import lru_cache

import numpy as np
import torch

from .. import _lib
from . import framecache
from .staging import Layout, StagedBatches, align as _align, copy_fills_device, copy_fills_host, default_decode as _default_decode, fills_behind

DESC = 20                                # MDCV_KPTLOAD_DESC
MIN_SIZE, MAX_SIZE, MAX_SIDE = 16, 256, 4096          # MDCV_KPTLOAD_MIN_SIZE / MAX_SIZE / MAX_SIDE
NUM_KPT = 7
_F32 = np.float32


def _default_probe(path):
    from PIL import Image
    with Image.open(path) as im:                             # the header only: no pixel is decoded
        return im.size


def _as_crop(img, what):
    crop = img if isinstance(img, np.ndarray) else np.asarray(img, dtype=np.uint8)
    if crop.ndim != 3 or crop.shape[2] != 3 or crop.dtype != np.uint8:
        raise ValueError(f"{what}: decode must give an (H, W, 3) uint8 RGB image, got {crop.shape} {crop.dtype}")
    return crop


# ------------------------------------------------------------------------------------------------------------------ the CSV
_CELL = r"^\s*\(([^,()]+),([^,()]+)\)\s*$"                 # a key-point cell: "(x,y)"


def _parse_table(table, keypoint_keys):
    """The labelled rows of the CSV -> (names [n] str, labels [n, len(keys), 2] float64)"""
    import pandas as pd
    keys = list(keypoint_keys)
    rows = table[table.iloc[:, 2].notna()]                   # an unlabelled row has no first label
    names = rows.iloc[:, 0].astype(str).to_numpy()
    cells = pd.Series(rows[keys].to_numpy(dtype=object).reshape(-1)).astype(str)
    xy = cells.str.extract(_CELL).apply(pd.to_numeric, errors="coerce").to_numpy(np.float64).reshape(len(rows), len(keys), 2)
    bad = np.isnan(xy).any(axis=(1, 2))
    if bad.any():
        raise ValueError(f"{names[bad][0]}: a key-point cell is not \"(x,y)\"")
    return names, xy


def _cached(folder):
    files = [os.path.join(folder, f) for f in ("images.npy", "labels.npy")]
    return files if all(os.path.exists(f) for f in files) else None


def load_train_csv_dataset(train_csv_uri, validation_percent, keypoint_keys, dataset_path, cache_location=None, decode=None):
    """RektNet/utils.py:152-235 -> (train_images, train_labels, val_images, val_labels): image names (column 0) and `[len(keys), 2]`
    float64 labels parsed from the "(x,y)" cells of the key-point columns.  Rows whose first label is NaN are skipped, then images whose
    decoded height is under 10; the first `int(n * validation_percent)` entries are the validation set.  With `cache_location` the two
    arrays are saved to / loaded from `<cache_location>/<sha256 of the table>/{images,labels}.npy` (no file is decoded on a hit)."""
    import pandas as pd
    table = pd.read_csv(train_csv_uri)
    folder = None
    if cache_location:
        folder = os.path.join(cache_location, hashlib.sha256(pd.util.hash_pandas_object(table, index=True).values).hexdigest())
    hit = _cached(folder) if folder else None
    if hit:
        print(f"key-point labels: read from the cache in {folder}")
        names, labels = np.load(hit[0]), np.load(hit[1])
    else:
        decode = decode or _default_decode
        names, labels = _parse_table(table, keypoint_keys)
        heights = np.array([_as_crop(decode(os.path.join(dataset_path, n)), n).shape[0] for n in names], np.int64)
        tall = heights >= 10
        names, labels = np.array([n.rsplit("/", 1)[-1] for n in names[tall]], dtype=str), labels[tall]
        if folder:
            os.makedirs(folder, exist_ok=True)
            np.save(os.path.join(folder, "images.npy"), names)
            np.save(os.path.join(folder, "labels.npy"), labels)
            print(f"key-point labels: cache written to {folder}")
    split = int(len(labels) * validation_percent)
    print(f"key-point labels: {len(labels) - split} training and {split} validation images")
    return names[split:], labels[split:], names[:split], labels[:split]


# ------------------------------------------------------------------------------------------------------------ labels (host, exact)
def scale_points(label, h, w, size):
    """`scale_labels(label, *get_scale((h, w), (size, size))) / size` (utils.py:98-111, dataset.py:41-43) -> float32 [n, 2]"""
    h_scale, w_scale = size / h, size / w
    out = np.empty((len(label), 2), np.float64)
    for k, pt in enumerate(np.array(label)):
        out[k, 0] = math.ceil(int(pt[0]) * w_scale) / size
        out[k, 1] = math.ceil(int(pt[1]) * h_scale) / size
    return out.astype(_F32)


def hot_pixels(label, h, w, name):
    """`(int(x), int(y))` per key point: where prep_label sets its one-hot.  Outside the h x w crop: IndexError naming the image."""
    hot = np.empty((len(label), 2), np.int32)
    for k, pt in enumerate(np.array(label)):
        x, y = int(pt[0]), int(pt[1])
        if not (0 <= x < w and 0 <= y < h):
            raise IndexError(f"{name}: key point {k} at ({pt[0]}, {pt[1]}) lies outside the {h}x{w} (h x w) crop")
        hot[k] = x, y
    return hot


@lru_cache(maxsize=4096)
def _read_mask(src, dst):
    """Which of `src` source samples a src -> dst INTER_LINEAR resize reads with a non-zero weight (bool [src]).  A one-hot at a sample
    no tap reads resizes to zeros, and prep_label's sum is 0: the host needs this only to print the reference's warning."""
    sc = float(src) / float(dst)
    fx = ((np.arange(dst, dtype=np.float64) + 0.5) * sc - 0.5).astype(_F32)
    sx = np.floor(fx).astype(np.int64)
    fx = (fx - sx.astype(_F32)).astype(_F32)
    lo, hi = sx < 0, sx >= src - 1
    sx[lo], fx[lo] = 0, 0
    sx[hi], fx[hi] = src - 1, 0
    mask = np.zeros(src, bool)
    mask[sx] = True                                         # weight 1 - fx > 0 always (fx < 1)
    s1 = np.minimum(sx + 1, src - 1)
    mask[s1[fx > 0]] = True
    return mask


def zero_sum_maps(hot, h, w, size):
    """-> bool [n]: key points whose heat-map sums to 0 before it is normalised (all NaN afterwards)"""
    mx, my = _read_mask(int(w), int(size)), _read_mask(int(h), int(size))
    return np.array([not (mx[x] and my[y]) for x, y in hot], bool)


# -------------------------------------------------------------------------------------------------------------------- the batch
def pack_layout(shapes):
    """Byte layout of one batch's staging buffer for crops of `shapes` [(h, w)]: [descriptors][points][pixels]"""
    p = Layout()
    p.B = len(shapes)
    p.desc_off, p.pts_off = 0, _align(p.B * DESC * 4)
    p.pix_off = _align(p.pts_off + p.B * NUM_KPT * 2 * 4)
    p.src_bytes = sum(3 * int(h) * int(w) for h, w in shapes)
    p.nbytes = _align(p.pix_off + p.src_bytes)
    return p


def pack_batch(buf, p, crops, hots, points, pooled=None, base=0):
    """Fill a uint8 numpy buffer of at least p.nbytes bytes (the pinned staging): crops [(h, w, 3) uint8] back to back, unaligned.
    With a frame cache, `pooled[b]` is (offset, h, w) for a crop that already lies in the pool (its entry of `crops` is None) and
    `base` is where the staged crops will lie in the same buffer: every descriptor's offset is then relative to the pool."""
    desc = buf[p.desc_off:p.desc_off + p.B * DESC * 4].view(np.int32).reshape(p.B, DESC)
    desc[:] = 0
    s = 0
    for b, (c, hot) in enumerate(zip(crops, hots)):
        desc[b, 4:4 + 2 * NUM_KPT] = np.asarray(hot, np.int32).reshape(-1)
        if c is None:
            desc[b, 0:3] = pooled[b]
            continue
        desc[b, 0:3] = base + s, c.shape[0], c.shape[1]
        n = c.shape[0] * c.shape[1] * 3
        buf[p.pix_off + s:p.pix_off + s + n] = c.reshape(-1)
        s += n
    buf[p.pts_off:p.pts_off + p.B * NUM_KPT * 8].view(np.float32)[:] = np.asarray(points, np.float32).reshape(-1)


def unpack_batch(buf, p):
    """The inverse of pack_batch on a host buffer -> (crops, hots [B,7,2], points [B,7,2]); tests and debugging."""
    desc = buf[p.desc_off:p.desc_off + p.B * DESC * 4].view(np.int32).reshape(p.B, DESC)
    crops = [buf[p.pix_off + o:p.pix_off + o + 3 * h * w].reshape(h, w, 3).copy() for o, h, w in desc[:, 0:3]]
    hots = desc[:, 4:4 + 2 * NUM_KPT].reshape(p.B, NUM_KPT, 2).copy()
    points = buf[p.pts_off:p.pts_off + p.B * NUM_KPT * 8].view(np.float32).reshape(p.B, NUM_KPT, 2).copy()
    return crops, hots, points


def check_size(target_image_size):
    """ConeDataset's `target_image_size` (a pair) or one int -> S; square, MIN_SIZE <= S <= MAX_SIZE"""
    if isinstance(target_image_size, (tuple, list)):
        if len(target_image_size) != 2 or int(target_image_size[0]) != int(target_image_size[1]):
            raise ValueError(f"ConeCropBatches: the target is square, got {tuple(target_image_size)}")
        target_image_size = target_image_size[0]
    size = int(target_image_size)
    if not MIN_SIZE <= size <= MAX_SIZE:
        raise ValueError(f"ConeCropBatches: target size {size} outside {MIN_SIZE}..{MAX_SIZE}")
    return size


def launch_batch(dev_buf, host_buf, p, size, stream, pool=None):
    """Enqueue csrc/kptload.hip's launch on `stream` for a staged batch already copied to `dev_buf` (device uint8)
    -> (imgs [B,3,S,S], heatmaps [B,7,S,S]).  `pool` (device uint8): the descriptors' offsets are relative to it, not to dev_buf's pixels."""
    L = _lib.lib()
    dev = dev_buf.device
    imgs = torch.empty(p.B, 3, size, size, dtype=torch.float32, device=dev)
    hm = torch.empty(p.B, NUM_KPT, size, size, dtype=torch.float32, device=dev)
    base = dev_buf.data_ptr()
    src, src_bytes = (base + p.pix_off, p.src_bytes) if pool is None else (pool.data_ptr(), int(pool.numel()))
    L.check(L.kptload_batch(host_buf.ctypes.data + p.desc_off, base + p.desc_off, p.B, src, src_bytes, size,
                            imgs.data_ptr(), hm.data_ptr(), stream.cuda_stream), "kptload_batch")
    return imgs, hm


def transform_batch(crops, labels, size, device=None, names=None):
    """Synchronous convenience (tests, probes): decoded crops [(h, w, 3) uint8 RGB] + their [7,2] labels
    -> (imgs [B,3,S,S], heatmaps [B,7,S,S], points [B,7,2]) fp32 on the device."""
    _lib.require_gpu()
    size = check_size(size)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    names = names if names is not None else [f"crop {b}" for b in range(len(crops))]
    crops = [_as_crop(c, n) for c, n in zip(crops, names)]
    hots = [hot_pixels(l, c.shape[0], c.shape[1], n) for l, c, n in zip(labels, crops, names)]
    points = [scale_points(l, c.shape[0], c.shape[1], size) for l, c in zip(labels, crops)]
    p = pack_layout([c.shape[:2] for c in crops])
    host = np.zeros(p.nbytes, np.uint8)
    pack_batch(host, p, crops, hots, points)
    with torch.cuda.device(device):
        dev = torch.from_numpy(host).to(device)
        imgs, hm = launch_batch(dev, host, p, size, torch.cuda.current_stream(device))
        pts = dev[p.pts_off:p.pts_off + p.B * NUM_KPT * 8].view(torch.float32).view(p.B, NUM_KPT, 2).clone()
    return imgs, hm, pts


class ConeCropBatches(StagedBatches):
    """Iterable of `(imgs [B,3,S,S], heatmaps [B,7,S,S], points [B,7,2], image_names, orig_sizes)`, the three tensors fp32 on the device:
    the batches that `DataLoader(ConeDataset(images, labels, dataset_path, target_image_size, ...), batch_size, shuffle=False)` yields.
    `image_names` is the list of `name.split(".")[0]`; `orig_sizes` is `[h, w, c]` as three int64 `[B]` tensors, what the default collate
    makes of `image.shape`.  File order, no shuffle, the last short batch kept; `len()` is the batch count, `len(.dataset)` the sample count.

    `images`, `labels`: what `load_train_csv_dataset` returns (names relative to `dataset_path`; `[7,2]` (x, y) labels in the pixels of
    the original crop).  `target_image_size`: S or (S, S), 16 <= S <= 256.  `decode(path)` -> a PIL image or an (H, W, 3) uint8 RGB
    array (default: `PIL.Image.open(path).convert('RGB')`), run on `num_workers` threads.  With `prefetch`, the next batches are decoded
    and staged while one is consumed.  `.incorrect_labels` collects the names whose labels give an all-NaN heat-map (module
    docstring).

    `cache_bytes`: None, or the HBM budget of a device-resident crop cache (mdcv/data/framecache.py): a crop is decoded
    once in the loader's lifetime and read from the pool afterwards; same outputs.  The label CSV has no sizes, so the constructor asks
    `probe(path)` -> (w, h) for each file (default: the image header through Pillow, no pixel decoded) and admits in file order.  The
    pool is the launch's `src`, whose offsets are `int`s: it ends below 2^31 bytes and crops beyond that are staged.  The budget bounds
    the cached crops; the allocation is larger by a tail, the bytes of the largest batch as probed, where a batch's staged crops lie
    under the same `src` (so `cache_bytes=0` allocates the tail and caches nothing).  A cached file that decodes to another size than
    probed is staged every time; a batch whose staged crops outgrow the tail, because uncached files decode larger than probed, raises
    ValueError.  `cache_stats()` counts what happened; `close()` frees the pool."""

    def __init__(self, images, labels, dataset_path, target_image_size, batch_size, decode=None, num_workers=None, device=None, prefetch=True,
                 cache_bytes=None, probe=None):
        if len(images) != len(labels):
            raise ValueError(f"ConeCropBatches: {len(images)} images for {len(labels)} labels")
        self.images = [str(n) for n in images]
        self.labels = [np.asarray(l, np.float64).reshape(-1, 2) for l in labels]
        for n, l in zip(self.images, self.labels):
            if l.shape != (NUM_KPT, 2):
                raise ValueError(f"{n}: {l.shape[0]} key points, the heat-map kernel takes {NUM_KPT}")
        self.dataset_path, self.size, self.batch_size = dataset_path, check_size(target_image_size), int(batch_size)
        if self.batch_size < 1:
            raise ValueError("ConeCropBatches: batch_size must be positive")
        self.dataset = range(len(self.images))
        self.incorrect_labels = []
        cache = None
        if cache_bytes is not None:
            probe = probe or _default_probe
            paths = [os.path.join(dataset_path, n) for n in self.images]
            known = {}
            for f in paths:
                if f not in known:
                    known[f] = tuple(int(v) for v in probe(f))
            sizes = [known[f] for f in paths]
            # behind the slots: room for one batch's staged crops, so that one `src` covers both kinds (one launch per batch)
            per = [sum(3 * w * h for w, h in sizes[i:i + self.batch_size]) for i in range(0, len(sizes), self.batch_size)]
            tail = framecache._round(max(per, default=0) + 1)
            cache = framecache.FrameCache(paths, sizes, cache_bytes, limit=(1 << 31) - 1 - tail, tail=tail)
        self._init_staging(num_workers, decode, prefetch, device, cache)

    def __len__(self):
        return (len(self.images) + self.batch_size - 1) // self.batch_size

    # -- host half: decode, labels, stage
    def _sample(self, index):
        """-> (crop or None, hot pixels, points, NaN-map flag, (h, w), cache entry or None): a cached crop has only its entry"""
        name = self.images[index]
        path = os.path.join(self.dataset_path, name)
        crop = ent = None
        if self._cache is not None:
            ent, crop = self._cache.lookup(path, lambda f: _as_crop(self.decode(f), name))
        else:
            crop = _as_crop(self.decode(path), name)
        h, w = crop.shape[:2] if ent is None else (ent.size[1], ent.size[0])
        if h > MAX_SIDE or w > MAX_SIDE:
            raise ValueError(f"{name}: a {h}x{w} crop is over the loader's bound of {MAX_SIDE} px a side")
        hot = hot_pixels(self.labels[index], h, w, name)
        return crop, hot, scale_points(self.labels[index], h, w, self.size), zero_sum_maps(hot, h, w, self.size).any(), (h, w), ent

    def _stage(self, bi, slot):
        idx = range(bi * self.batch_size, min(len(self.images), (bi + 1) * self.batch_size))
        got = self._map(self._sample, idx)
        for i, g in zip(idx, got):
            if g[3]:
                print("Incorrect Data Label Detected! Please revise the image label below and becoming the one with data!")
                print(self.images[i])
                if self.images[i] not in self.incorrect_labels:
                    self.incorrect_labels.append(self.images[i])
        crops, ents = [g[0] for g in got], [g[5] for g in got]
        p = pack_layout([(0, 0) if c is None else c.shape[:2] for c in crops])
        fills, pooled, base = [], None, 0
        if self._cache is not None:
            c = self._cache
            base = c.bytes_reserved                              # the tail of the pool: this batch's staged crops
            if p.src_bytes > c.tail:
                raise ValueError(f"batch {bi}: {p.src_bytes} bytes of staged crops, the cache planned for {c.tail} (a file decodes larger "
                                 f"than `probe` said)")
            pooled = [None if e is None else (e.offset, e.size[1], e.size[0]) for e in ents]
            fills = c.take_fills(ents)
        p.fills, need = fills_behind(p.nbytes, fills)            # first sight: the whole crops ride behind the batch, one copy each
        host = slot.buffer(need).numpy()
        pack_batch(host, p, crops, [g[1] for g in got], [g[2] for g in got], pooled, base)
        copy_fills_host(host, p.fills)
        names = [self.images[i].split(".")[0] for i in idx]
        sizes = [torch.tensor([hw[0] for hw in (g[4] for g in got)], dtype=torch.int64),
                 torch.tensor([hw[1] for hw in (g[4] for g in got)], dtype=torch.int64), torch.full((len(got),), 3, dtype=torch.int64)]
        return names, sizes, p, slot

    # -- device half: one H2D copy and the launch on the side stream
    def _enqueue(self, staged):
        names, sizes, p, slot = staged
        dev = self.device
        with torch.cuda.device(dev), torch.cuda.stream(self._stream):
            pool = None
            if self._cache is None:
                dbuf = torch.empty(p.nbytes, dtype=torch.uint8, device=dev)
                dbuf.copy_(slot.pinned[:p.nbytes], non_blocking=True)
            else:                                                # descriptors and points to the batch's buffer, every pixel to the pool
                pool, tail = self._cache.pool, self._cache.bytes_reserved
                dbuf = torch.empty(p.pix_off, dtype=torch.uint8, device=dev)
                dbuf.copy_(slot.pinned[:p.pix_off], non_blocking=True)
                if p.src_bytes:
                    pool[tail:tail + p.src_bytes].copy_(slot.pinned[p.pix_off:p.pix_off + p.src_bytes], non_blocking=True)
                copy_fills_device(pool, slot.pinned, p.fills)
            self._copied(slot, p.fills)
            imgs, hm = launch_batch(dbuf, slot.pinned.numpy(), p, self.size, self._stream, pool)
            pts = dbuf[p.pts_off:p.pts_off + p.B * NUM_KPT * 8].view(torch.float32).view(p.B, NUM_KPT, 2).clone()
            return imgs, hm, pts, names, sizes, self._ready()     # the next epoch waits for it: this launch reads the pool's tail

    def __iter__(self):
        _lib.require_gpu()
        yield from self._batches(len(self), self._stage)
