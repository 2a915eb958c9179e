"""Batched image and frame detection with the boxes drawn on the device: the native counterpart of CVC-YOLOv3/detect.py.

The reference's `single_img_detect` (detect.py:60-111) costs, per frame, a Pillow pad and resize on the host, a batch-1 forward, four
`.item()` reads per kept box (:100-103) and a host `ImageDraw.rectangle` (:104).  `FrameDetector.detect_frames` runs the same steps over
batches of decoded frames that stay on the device from the upload to the annotated pixels:

  1. the whole frames of a batch are packed into one pinned buffer at 16-byte-aligned offsets, behind the resize descriptors and tables,
  2. one H2D copy; the frames' bytes on the device are the batch's frame pool,
  3. pad-and-resize reads each frame in place from that pool (`sample_geometry(ts=False)`, `mdcv_imgload_frames_batch`: the loaders'
     byte-exact Pillow resize, nothing new),
  4. `model.eval()`, forward under `no_grad`,
  5. `detect_postprocess(output, None, ...)`: confidence filter and NMS of the whole batch, no host round trip,
  6. `mdcv_detect_draw_boxes` (csrc/detect_draw.hip) on the same stream into the same pool bytes: each kept box mapped to frame
     coordinates in IEEE double as detect.py:100-103 maps it, truncated as Pillow truncates it, and outlined as Pillow 12.2 outlines it,
  7. one D2H copy of the pool and the small tables behind it,

with ONE host synchronisation per batch and none per box.  Two staging slots: batch n + 1 is taken from the iterable and packed (on a
worker thread) while the device works on batch n.

`FrameConeDetector` carries the same batches on to the key points of every cone (crops cut from the pool, one batched KeypointNet eval,
outlines and key-point discs drawn on the device).

`TiledFrameDetector` / `TiledFrameConeDetector` run the same interface on the tiles training sees (`ts=True`): every tile at its native
scale through the network, the tiles' detections merged per frame by `mdcv_detect_merge_tiles` (csrc/detect_tiles.hip).

`single_img_detect` and `detect` take the reference's argument lists, so a caller swaps the import.  Departures, all
documented in DESIGN.md §19: a box Pillow would refuse (x1 < x0, y1 < y0) or C could not convert (NaN, inf, magnitude >= 2^30) is skipped
and counted instead of raising; a file whose Pillow mode is not RGB raises ValueError (the reference draws on the unconverted image and
its ink then depends on the mode); with no detection the unannotated image is saved (the reference hits an unbound variable); video
containers need cv2 and raise ValueError; `detect` also accepts a directory of images, the batched stand-in for the frame-dump video loop.
"""
import os
from concurrent.futures import ThreadPoolExecutor
from itertools import islice

import numpy as np
import torch

from .. import _lib
from ..data import images as I
from ..data import staging
from .postprocess import detect_postprocess, L_MAX_TOPK

DETECT_DESC = 6                          # MDCV_DETECT_DESC
IMG_FORMATS = (".jpg", ".jpeg", ".png", ".tif")         # detect.py:122-123
VID_FORMATS = (".mov", ".avi", ".mp4")
_align = staging.align


# ------------------------------------------------------------------------------------------------------------- host layout (no GPU)
def frame_offsets(sizes):
    """[(W, H)] -> ([byte offset of each whole frame in the pool, 16-byte aligned], pool bytes)"""
    offsets, at = [], 0
    for w, h in sizes:
        offsets.append(at)
        at = _align(at + 3 * int(w) * int(h))
    return offsets, at


def detect_descriptors(geoms, offsets):
    """MDCV_DETECT_DESC long longs per frame (include/mdcv_hip.h): off, W, H, the bits of the double `ratio`, pad_w, pad_h -- ratio and
    pads are `letterbox()`'s, as the pad-and-resize geometry carries them"""
    d = np.zeros((len(geoms), DETECT_DESC), np.int64)
    for b, (g, off) in enumerate(zip(geoms, offsets)):
        d[b, 0], d[b, 1], d[b, 2] = off, g.frame[0], g.frame[1]
        d[b, 3] = np.array([g.ratio], np.float64).view(np.int64)[0]
        d[b, 4], d[b, 5] = g.pad_w, g.pad_h
    return d


class BatchPlan:
    """Byte layout of one batch.  Device buffer: [resize descriptors, tables and frame references (images.pack_layout)] [detect
    descriptors] [pool: the whole frames] [frame_boxes B,K,4 f64] [rects B,K,4 i32] [prob B,K f32] [count B i32] [skipped B i32];
    the pinned input is everything up to the end of the pool, the copy back is everything from the pool (or from the tables) on.
    Subclasses choose the resize samples (`_samples`) and may put input tables behind the detect descriptors (`_tables`)."""

    src_off = None                           # tiled plans: [src B,K,2 i32] behind the tables

    def __init__(self, sizes, width, height, K):
        B = len(sizes)
        self.B, self.K, self.sizes = B, int(K), [(int(w), int(h)) for w, h in sizes]
        self.offsets, self.pool_bytes = frame_offsets(self.sizes)
        self._samples(width, height)
        self.layout = I.pack_layout(self.geoms, [0] * len(self.geoms), 0, self.frefs)
        self.det_off = self.layout.nbytes
        self.pool_off = _align(self._tables(self.det_off + B * DETECT_DESC * 8))
        self.in_bytes = self.pool_off + self.pool_bytes
        self.fb_off = self.in_bytes                                          # 16-byte aligned: pool_off and pool_bytes both are
        self.rect_off = self.fb_off + B * self.K * 32
        self.prob_off = self.rect_off + B * self.K * 16
        self.count_off = _align(self.prob_off + B * self.K * 4)
        self.skip_off = _align(self.count_off + B * 4)
        self.nbytes = _align(self.skip_off + B * 4)

    def _samples(self, width, height):
        """the resize samples of the batch (geoms, frefs: one per network input) and the detect descriptors (one per frame)"""
        self.geoms = [I.sample_geometry(w, h, width, height, ts=False) for w, h in self.sizes]
        self.frefs = [I.frame_reference(g, o) for g, o in zip(self.geoms, self.offsets)]
        self.desc = detect_descriptors(self.geoms, self.offsets)

    def _tables(self, at):
        """input tables behind the detect descriptors, which end at byte `at` -> where they end"""
        return at

    def _pack_tables(self, host):
        pass

    def pack(self, host, frames):
        """fill the pinned input (uint8 numpy, >= in_bytes) with the batch"""
        I.pack_batch(host, self.layout, self.geoms, [None] * len(self.geoms), frefs=self.frefs)
        host[self.det_off:self.det_off + self.desc.nbytes].view(np.int64)[:] = self.desc.reshape(-1)
        self._pack_tables(host)
        for f, off, (w, h) in zip(frames, self.offsets, self.sizes):
            host[self.pool_off + off:self.pool_off + off + 3 * w * h] = f.reshape(-1)


TILE_DESC = 4                            # MDCV_TILE_DESC
MAX_TILES_PER_FRAME = 64                 # MDCV_TILE_MAX_PER_FRAME


def tiled_descriptors(sizes, offsets, scales):
    """MDCV_DETECT_DESC long longs per frame for tile-and-scale inference: a merged box is in scaled-frame pixels, so `ratio` is the
    frame's scale (its float64 bits) and both pads are 0 -- mdcv_detect_map_boxes / _draw_boxes then compute x / scale, the inverse of
    the training labels' scale_labels step"""
    d = np.zeros((len(sizes), DETECT_DESC), np.int64)
    for b, ((w, h), off, s) in enumerate(zip(sizes, offsets, scales)):
        d[b, 0], d[b, 1], d[b, 2] = off, w, h
        d[b, 3] = np.array([s], np.float64).view(np.int64)[0]
    return d


class TiledBatchPlan(BatchPlan):
    """BatchPlan for tile-and-scale inference: frame b is scaled by scales[b] and cut into its `n_patches` network-sized tiles, exactly
    the `sample_geometry(ts=True)` patches training sees.  Every tile is one resize sample with a frame reference into the batch's pool
    (the tiles are resized from the pool bytes in place, nothing is staged twice).  Behind the detect descriptors lies the tile table
    of mdcv_detect_merge_tiles, TILE_DESC int32 per tile: (frame, off_x, off_y, 0) with off = the rounded patch origin minus the
    border, the same rounding `sample_geometry` applies; behind the output tables, [src B,K,2 i32].  `first`: the index of the
    batch's first frame in the caller's sequence, for error messages."""

    def __init__(self, sizes, width, height, K, scales, first=0):
        self.scales = [float(s) for s in scales]
        if len(self.scales) != len(sizes):
            raise ValueError(f"TiledBatchPlan: {len(sizes)} frames but {len(self.scales)} scales")
        self.first = int(first)
        super().__init__(sizes, width, height, K)
        self.src_off = self.nbytes
        self.nbytes = _align(self.src_off + self.B * self.K * 8)

    def _samples(self, width, height):
        self.geoms, self.frefs, self.tile_frame, table = [], [], [], []
        for b, ((w, h), s, off) in enumerate(zip(self.sizes, self.scales, self.offsets)):
            try:
                if not 0.0 < s < float(1 << 30):
                    raise ValueError(f"scale must be positive and below 2^30, got {s}")
                tiles = [I.sample_geometry(w, h, width, height, ts=True, scale=s)]
                n = tiles[0].n_patches
                if n > MAX_TILES_PER_FRAME:
                    raise ValueError(f"scale {s} cuts a {w}x{h} frame into {n} tiles of {width}x{height}, more than {MAX_TILES_PER_FRAME}")
                tiles += [I.sample_geometry(w, h, width, height, ts=True, scale=s, patch_index=i) for i in range(1, n)]
            except ValueError as e:
                raise ValueError(f"frame {self.first + b}: {e}") from None
            for g in tiles:
                self.geoms.append(g)
                self.frefs.append(I.frame_reference(g, off))
                self.tile_frame.append(b)
                table.append((b, int(round(g.boundary[0])) - g.hp, int(round(g.boundary[1])) - g.vp, 0))
        self.NT = len(self.geoms)
        self.tile_table = np.asarray(table, np.int32).reshape(self.NT, TILE_DESC)
        self.desc = tiled_descriptors(self.sizes, self.offsets, self.scales)

    def _tables(self, at):
        self.tile_off = _align(at)
        return self.tile_off + self.NT * TILE_DESC * 4

    def _pack_tables(self, host):
        host[self.tile_off:self.tile_off + self.tile_table.nbytes].view(np.int32)[:] = self.tile_table.reshape(-1)


def _check_frame(f, i):
    f = np.asarray(f)
    if f.ndim != 3 or f.shape[2] != 3 or f.dtype != np.uint8 or f.shape[0] < 1 or f.shape[1] < 1:
        raise ValueError(f"detect_frames: frame {i} must be an (H, W, 3) uint8 RGB array, got {f.shape} {f.dtype}")
    return np.ascontiguousarray(f)


class FrameDetections:
    """One frame's result.  boxes float64 [n,4] (x0, y0, x1, y1 in frame coordinates, most confident first), prob float32 [n], rects int32
    [n,4] (the truncated boxes as drawn; (0, 0, -1, -1) for a skipped one), skipped (boxes not drawn), annotated (H, W, 3) uint8 -- a
    NumPy array, or a device tensor with `keep_on_device`."""

    __slots__ = ("boxes", "prob", "rects", "skipped", "annotated")

    def __init__(self, boxes, prob, rects, skipped, annotated):
        self.boxes, self.prob, self.rects, self.skipped, self.annotated = boxes, prob, rects, skipped, annotated


class TiledFrameDetections(FrameDetections):
    """FrameDetections of a tiled detector, and src int32 [n,2]: per box the tile it came from (its index among the tiles of the
    batch, frames in order, a frame's tiles row-major over its grid) and its slot in that tile's detections."""

    __slots__ = ("src",)


class _Slot:
    def __init__(self):
        self.pin_in, self.pin_out, self.pin_total = None, None, None


class FrameDetector:
    """`FrameDetector(model).detect_frames(frames)`: see the module docstring.  conf_thres / nms_thres default to `model.get_threshs()`;
    at most `max_boxes` (<= top_k) boxes per frame are mapped and drawn, the most confident ones; `outline` is the one RGB triple of a
    call (default `ImageColor.getrgb("red")`).  Subclasses override `_plan` (the batch's layout), `_batch_boxes` (the boxes of a batch) and
    `_result_type`; FrameConeDetector also `_annotate` and `_extras`; everything else -- staging, the copy back, the final synchronisation -- is shared."""

    _result_type = FrameDetections

    def __init__(self, model, conf_thres=None, nms_thres=None, top_k=200, max_boxes=200, outline=(255, 0, 0), batch_size=16):
        conf, nms, _ = model.get_threshs()
        self.model = model
        self.conf_thres = float(conf if conf_thres is None else conf_thres)
        self.nms_thres = float(nms if nms_thres is None else nms_thres)
        self.top_k, self.max_boxes, self.batch_size = int(top_k), int(max_boxes), int(batch_size)
        if not 0 < self.top_k <= L_MAX_TOPK or not 0 < self.max_boxes <= self.top_k:
            raise ValueError(f"FrameDetector: need 0 < max_boxes <= top_k <= {L_MAX_TOPK}, got max_boxes {max_boxes}, top_k {top_k}")
        if self.batch_size < 1:
            raise ValueError(f"FrameDetector: batch_size must be positive, got {batch_size}")
        self.outline = tuple(int(c) for c in outline)
        if len(self.outline) != 3 or any(not 0 <= c <= 255 for c in self.outline):
            raise ValueError(f"FrameDetector: outline must be one RGB triple of bytes, got {outline!r}")
        self.bw = bool(model.get_bw())
        self.width, self.height = (int(v) for v in model.img_size())

    @property
    def device(self):
        return next(self.model.parameters()).device

    # -- host half (worker thread): take a batch from the iterable, plan it, pack it into the slot's pinned buffer
    def _plan(self, sizes, first):
        return BatchPlan(sizes, self.width, self.height, self.top_k)

    def _stage(self, it, first, slot):
        frames = [_check_frame(f, first + i) for i, f in enumerate(islice(it, self.batch_size))]
        if not frames:
            return None
        plan = self._plan([(f.shape[1], f.shape[0]) for f in frames], first)
        slot.pin_in = staging.pinned(slot.pin_in, plan.in_bytes)
        plan.pack(slot.pin_in.numpy(), frames)
        return plan, slot

    # -- the boxes of a batch, enqueued on `st`: resize from the pool, eval forward, post-process -> device tensors boxes [B,K,4] fp32 in
    #    the coordinates the plan's detect descriptors map from, prob [B,K], count [B] int32 (capped at max_boxes), src [B,K,2] or None
    def _batch_boxes(self, plan, dbuf, host, pool, st):
        imgs = I.launch_batch(dbuf, host, plan.layout, 1 if self.bw else 3, self.height, self.width, st, pool)
        self.model.eval()
        det = detect_postprocess(self.model(imgs), None, self.conf_thres, self.nms_thres, 0.5, self.width, self.height, self.top_k)
        count = det.count if self.max_boxes >= self.top_k else det.count.clamp(max=self.max_boxes)
        return det.boxes, det.prob, count, None

    def _draw_boxes(self, plan, dbuf, host, boxes, count, st):
        L, base = _lib.lib(), dbuf.data_ptr()
        L.check(L.detect_draw_boxes(host.ctypes.data + plan.det_off, base + plan.det_off, plan.B, boxes.data_ptr(), count.data_ptr(), plan.K,
                                    base + plan.pool_off, plan.pool_bytes, *self.outline, base + plan.fb_off, base + plan.rect_off,
                                    base + plan.skip_off, st.cuda_stream), "detect_draw_boxes")

    # -- what is enqueued between the boxes and the copy back -> whatever `_extras` needs
    def _annotate(self, plan, slot, dbuf, host, boxes, count, st):
        self._draw_boxes(plan, dbuf, host, boxes, count, st)

    # -- behind the final synchronisation -> add(r, b, n): what a subclass adds to frame b's result r with its n boxes
    def _extras(self, plan, table, annotated):
        return lambda r, b, n: None

    # -- device half: copy, boxes, draw, copy back, ONE synchronisation
    def _run(self, plan, slot, keep_on_device):
        dev = self.device
        B, K = plan.B, plan.K
        with torch.cuda.device(dev), torch.no_grad():
            st = torch.cuda.current_stream(dev)
            dbuf = staging.upload(slot.pin_in, plan.in_bytes, plan.nbytes, dev)
            pool = dbuf[plan.pool_off:plan.pool_off + plan.pool_bytes]
            host = slot.pin_in.numpy()
            boxes, bprob, count, src = self._batch_boxes(plan, dbuf, host, pool, st)
            annotated = self._annotate(plan, slot, dbuf, host, boxes, count, st)
            dbuf[plan.prob_off:plan.prob_off + B * K * 4].view(torch.float32).copy_(bprob.reshape(-1))
            dbuf[plan.count_off:plan.count_off + B * 4].view(torch.int32).copy_(count)
            if src is not None:
                dbuf[plan.src_off:plan.src_off + B * K * 8].view(torch.int32).copy_(src.reshape(-1))
            lo = plan.fb_off if keep_on_device else plan.pool_off
            slot.pin_out, table = staging.copy_back(dbuf, lo, slot.pin_out, st)       # the batch's one (or last) host synchronisation
            add = self._extras(plan, table, annotated)
        fb = table(plan.fb_off, B * K * 32, np.float64, (B, K, 4))
        rects = table(plan.rect_off, B * K * 16, np.int32, (B, K, 4))
        prob = table(plan.prob_off, B * K * 4, np.float32, (B, K))
        cnt = table(plan.count_off, B * 4, np.int32, (B,))
        skipped = table(plan.skip_off, B * 4, np.int32, (B,))
        res = []
        for b, (off, (w, h)) in enumerate(zip(plan.offsets, plan.sizes)):
            n = min(int(cnt[b]), K)
            if keep_on_device:
                ann = pool[off:off + 3 * w * h].view(h, w, 3)
            else:
                ann = table(plan.pool_off + off, 3 * w * h, np.uint8, (h, w, 3)).copy()      # the pinned buffer is the next batch's
            r = self._result_type(fb[b, :n].copy(), prob[b, :n].copy(), rects[b, :n].copy(), int(skipped[b]), ann)
            if plan.src_off is not None:
                r.src = table(plan.src_off, B * K * 8, np.int32, (B, K, 2))[b, :n].copy()
            add(r, b, n)
            res.append(r)
        return res

    def detect_frames(self, frames, keep_on_device=False):
        """frames: any iterable of (H, W, 3) uint8 RGB arrays (sizes may differ inside a batch) -> yields one `FrameDetections` per frame, in
        order.  keep_on_device: `annotated` is a device tensor (a view of the batch's device buffer) and no pixel is copied back."""
        _lib.require_gpu()
        it = iter(frames)
        slots = [_Slot(), _Slot()]                               # this generator's own: several may be alive on one detector
        stager = ThreadPoolExecutor(1, thread_name_prefix="mdcv-detect-stage")
        try:
            n, first = 0, 0
            pending = stager.submit(self._stage, it, first, slots[0])
            while True:
                staged = pending.result()
                if staged is None:
                    break
                n += 1
                first += staged[0].B
                pending = stager.submit(self._stage, it, first, slots[n % 2])     # packed while the device works on this batch
                yield from self._run(*staged, keep_on_device)
        finally:
            stager.shutdown(wait=True, cancel_futures=True)


# ------------------------------------------------------------------------------------ frames -> boxes -> crops -> key points, drawn
# RektNet/utils.py:62's BGR triples reversed: the pool is RGB, so the picture shows the reference's colours
KPT_COLOURS_RGB = ((0, 255, 0), (0, 0, 255), (0, 255, 255), (255, 255, 0), (255, 0, 255), (127, 255, 127), (127, 127, 255))
NUM_KPT = 7


def colour_table(colours):
    """seven RGB triples -> the contiguous 7 x 3 uint8 table mdcv_kpt_draw_points takes (a host array)"""
    t = np.ascontiguousarray(colours, dtype=np.int64)
    if t.shape != (NUM_KPT, 3) or (t < 0).any() or (t > 255).any():
        raise ValueError(f"key-point colours must be {NUM_KPT} RGB triples of bytes, got {colours!r}")
    return np.ascontiguousarray(t, dtype=np.uint8)


def padded_rows(M, bucket):
    """rows of the key-point batch for M crops: the next multiple of `bucket` (as JointPipeline pads), 0 for none"""
    return (M + bucket - 1) // bucket * bucket


class ConeBatchPlan(BatchPlan):
    """BatchPlan with the cone tables behind it: [total 1 i32] [owner cap,2 i32] [window cap,4 i32] [keypoints cap,7,2 f32]
    [centers cap,7,2 i32] [skipped points B i32], cap = B * per rows, per = min(max_cones, K) crops per frame at most."""

    def __init__(self, sizes, width, height, K, max_cones):
        super().__init__(sizes, width, height, K)
        _append_cone_tables(self, max_cones)


def _append_cone_tables(plan, max_cones):
    plan.per = min(int(max_cones), plan.K)
    plan.cap = cap = plan.B * plan.per
    plan.total_off = plan.nbytes
    plan.owner_off = plan.total_off + 16
    plan.window_off = _align(plan.owner_off + cap * 8)
    plan.pts_off = _align(plan.window_off + cap * 16)
    plan.centers_off = _align(plan.pts_off + cap * NUM_KPT * 8)
    plan.kskip_off = _align(plan.centers_off + cap * NUM_KPT * 8)
    plan.nbytes = _align(plan.kskip_off + plan.B * 4)


class TiledConeBatchPlan(TiledBatchPlan):
    """TiledBatchPlan with ConeBatchPlan's tables behind it"""

    def __init__(self, sizes, width, height, K, scales, max_cones, first=0):
        super().__init__(sizes, width, height, K, scales, first)
        _append_cone_tables(self, max_cones)


def scatter_cones(owner, pts, centers, b, n):
    """the rows of frame b among a batch's cone tables (owner [M,2] = (frame, slot)) -> per-box arrays for its n boxes:
    keypoints [n,7,2] float32 (NaN without a crop), keypoints_frame [n,7,2] int32 ((-1, -1) without), has_crop [n] bool"""
    kp = np.full((n, NUM_KPT, 2), np.nan, np.float32)
    kf = np.full((n, NUM_KPT, 2), -1, np.int32)
    has = np.zeros(n, bool)
    rows = np.nonzero(owner[:, 0] == b)[0]
    slots = owner[rows, 1]
    kp[slots], kf[slots], has[slots] = pts[rows], centers[rows], True
    return kp, kf, has, rows


class FrameCones(FrameDetections):
    """One frame's result: FrameDetections' fields, and per box keypoints float32 [n,7,2] (x, y normalised in the crop; NaN for a box
    without a crop), keypoints_frame int32 [n,7,2] (the disc centres as drawn, in frame pixels; (-1, -1) for a box without a crop or a
    point that was skipped), has_crop bool [n], skipped_points (key points of this frame not drawn), and crops (float32 [c,3,S,S], the
    KeypointNet inputs of the boxes with a crop in box order; None unless asked for)."""

    __slots__ = ("keypoints", "keypoints_frame", "has_crop", "skipped_points", "crops")


class FrameConeDetector(FrameDetector):
    """`FrameConeDetector(model, keypoint_net).detect_frames(frames)`: FrameDetector's batches carried on to the key points of every cone,
    everything between the upload and the annotated pixels on the device.  Per batch, on one stream: upload, pad-and-resize
    from the pool, eval forward, `detect_postprocess`, the box mapping (`mdcv_detect_map_boxes`: FrameDetector's frame_boxes and rects,
    no pixel touched), `mdcv_crop_resize_frames_u8` (every kept box's clipped window cut out of the untouched frame in the pool and resized
    as RektNet's loaders resize, at most `max_cones` per frame), one batched `keypoint_net` eval on the crops, the box outlines
    (`mdcv_detect_draw_boxes`), the key-point discs on top (`mdcv_kpt_draw_points`, `colours`: seven RGB triples), one D2H copy.

    TWO host synchronisations per batch and none per box or cone: the crop total (it sizes the key-point batch, padded with zero rows to
    a multiple of `bucket` as JointPipeline pads) and the end.  A batch without a crop skips the key-point forward.
    `detect_frames(..., return_crops=True)` also copies the crops back (a third synchronisation; tests and debugging)."""

    def __init__(self, model, keypoint_net, conf_thres=None, nms_thres=None, top_k=200, max_boxes=200, outline=(255, 0, 0), batch_size=16,
                 max_cones=64, bucket=64, colours=KPT_COLOURS_RGB):
        super().__init__(model, conf_thres, nms_thres, top_k, max_boxes, outline, batch_size)
        self.keypoint_net = keypoint_net
        self.max_cones, self.bucket = int(max_cones), int(bucket)
        if self.max_cones < 1 or self.bucket < 1:
            raise ValueError(f"FrameConeDetector: max_cones and bucket must be positive, got {max_cones}, {bucket}")
        size = tuple(int(v) for v in keypoint_net.image_size)
        if size[0] != size[1] or not 16 <= size[0] <= 256:                    # MDCV_KPTLOAD_MIN_SIZE / MAX_SIZE
            raise ValueError(f"FrameConeDetector: the key-point input must be square with a side in 16..256, got {size}")
        if int(getattr(keypoint_net, "num_kpt", NUM_KPT)) != NUM_KPT:
            raise ValueError(f"FrameConeDetector: the drawing kernel takes {NUM_KPT} key points per cone")
        self.size = size[0]
        self.colours = colour_table(colours)
        self._return_crops = False

    _result_type = FrameCones

    def _plan(self, sizes, first):
        return ConeBatchPlan(sizes, self.width, self.height, self.top_k, self.max_cones)

    def _annotate(self, plan, slot, dbuf, host, boxes, count, st):
        L = _lib.lib()
        B, K, S = plan.B, plan.K, self.size
        base = dbuf.data_ptr()
        desc_h, desc_d = host.ctypes.data + plan.det_off, base + plan.det_off
        L.check(L.detect_map_boxes(desc_h, desc_d, B, boxes.data_ptr(), count.data_ptr(), K, plan.pool_bytes, base + plan.fb_off,
                                   base + plan.rect_off, base + plan.skip_off, st.cuda_stream), "detect_map_boxes")
        crops = torch.empty(max(padded_rows(plan.cap, self.bucket), 1), 3, S, S, dtype=torch.float32, device=dbuf.device)
        L.check(L.crop_resize_frames_u8(desc_h, desc_d, B, base + plan.pool_off, plan.pool_bytes, base + plan.rect_off, count.data_ptr(), K,
                                        plan.per, S, crops.data_ptr(), base + plan.owner_off, base + plan.window_off,
                                        base + plan.total_off, st.cuda_stream), "crop_resize_frames_u8")
        if slot.pin_total is None:
            slot.pin_total = staging.pinned(None, 16, 16).view(torch.int32)
        slot.pin_total.copy_(dbuf[plan.total_off:plan.total_off + 16].view(torch.int32), non_blocking=True)
        sized = torch.cuda.Event()
        sized.record(st)
        sized.synchronize()                                      # synchronisation 1 of 2: the crop total sizes the key-point batch
        M = int(slot.pin_total.numpy()[0])
        if M:
            rows = padded_rows(M, self.bucket)
            crops[M:rows].zero_()
            self.keypoint_net.eval()
            _hm, pts = self.keypoint_net(crops[:rows])
            dbuf[plan.pts_off:plan.pts_off + M * NUM_KPT * 8].view(torch.float32).copy_(pts[:M].reshape(-1))
        self._draw_boxes(plan, dbuf, host, boxes, count, st)
        L.check(L.kpt_draw_points(desc_h, desc_d, B, base + plan.pool_off, plan.pool_bytes, base + plan.pts_off, base + plan.window_off,
                                  base + plan.owner_off, M, self.colours.ctypes.data, base + plan.centers_off, base + plan.kskip_off,
                                  st.cuda_stream), "kpt_draw_points")
        return M, crops

    def _extras(self, plan, table, annotated):
        M, crops = annotated
        crops_host = crops[:M].cpu().numpy() if self._return_crops else None
        owner = table(plan.owner_off, M * 8, np.int32, (M, 2))
        kpts = table(plan.pts_off, M * NUM_KPT * 8, np.float32, (M, NUM_KPT, 2))
        centers = table(plan.centers_off, M * NUM_KPT * 8, np.int32, (M, NUM_KPT, 2))
        kskip = table(plan.kskip_off, plan.B * 4, np.int32, (plan.B,))

        def add(r, b, n):
            r.keypoints, r.keypoints_frame, r.has_crop, rows = scatter_cones(owner, kpts, centers, b, n)
            r.skipped_points = int(kskip[b])
            r.crops = crops_host[rows] if crops_host is not None else None
        return add

    def detect_frames(self, frames, keep_on_device=False, return_crops=False):
        """as FrameDetector.detect_frames -> yields one `FrameCones` per frame, in order"""
        self._return_crops = bool(return_crops)
        return super().detect_frames(frames, keep_on_device)


# ------------------------------------------------------------------------------------------------- tile-and-scale inference
class TiledFrameCones(FrameCones):
    """FrameCones of a tiled detector, and src int32 [n,2] as in TiledFrameDetections"""

    __slots__ = ("src",)


class _Tiled:
    """The tiled front of a detector: the frame is scaled and cut into the tiles training sees (`ImageLabelBatches(ts=True)`), every tile
    goes through the network at its native size, and mdcv_detect_merge_tiles (csrc/detect_tiles.hip) makes the tiles' detections one list
    per frame.  Per batch, on the detector's one stream: all tiles resized from the pool in one launch, the eval forward and
    `detect_postprocess` in chunks of `tile_batch` tiles, ONE merge launch -- no count is read by the host."""

    def _init_tiles(self, scale, tile_batch, contain_thres):
        if not callable(scale):
            value = float(scale)
            scale = lambda w, h: value                                       # noqa: E731
        self.scale = scale
        self.tile_batch = int(tile_batch)
        if self.tile_batch < 1:
            raise ValueError(f"{type(self).__name__}: tile_batch must be positive, got {tile_batch}")
        self.contain_thres = -1.0 if contain_thres is None else float(contain_thres)      # negative: the seam rule is off
        if contain_thres is not None and not self.contain_thres >= 0.0:
            raise ValueError(f"{type(self).__name__}: contain_thres must be None or >= 0, got {contain_thres}")

    def _scales(self, sizes):
        return [float(self.scale(w, h)) for w, h in sizes]

    def _batch_boxes(self, plan, dbuf, host, pool, st):
        L = _lib.lib()
        B, K, NT = plan.B, plan.K, plan.NT
        imgs = I.launch_batch(dbuf, host, plan.layout, 1 if self.bw else 3, self.height, self.width, st, pool)      # [NT,C,H,W]
        self.model.eval()
        dets = [detect_postprocess(self.model(imgs[at:at + self.tile_batch]), None, self.conf_thres, self.nms_thres, 0.5, self.width,
                                   self.height, self.top_k) for at in range(0, NT, self.tile_batch)]
        one = len(dets) == 1
        tboxes = dets[0].boxes if one else torch.cat([d.boxes for d in dets])
        tprob = dets[0].prob if one else torch.cat([d.prob for d in dets])
        tcount = dets[0].count if one else torch.cat([d.count for d in dets])
        dev = dbuf.device
        boxes = torch.empty(B, K, 4, dtype=torch.float32, device=dev)        # the kernel writes every entry (zeros past count[b])
        prob = torch.empty(B, K, dtype=torch.float32, device=dev)
        src = torch.empty(B, K, 2, dtype=torch.int32, device=dev)
        count = torch.empty(B, dtype=torch.int32, device=dev)
        L.check(L.detect_merge_tiles(tboxes.data_ptr(), tprob.data_ptr(), tcount.data_ptr(), host.ctypes.data + plan.tile_off,
                                     dbuf.data_ptr() + plan.tile_off, NT, K, B, self.nms_thres, self.contain_thres, K, boxes.data_ptr(),
                                     prob.data_ptr(), src.data_ptr(), count.data_ptr(), st.cuda_stream), "detect_merge_tiles")
        if self.max_boxes < self.top_k:
            count = count.clamp(max=self.max_boxes)
        return boxes, prob, count, src


class TiledFrameDetector(_Tiled, FrameDetector):
    """`TiledFrameDetector(model, scale).detect_frames(frames)`: FrameDetector's interface on the tiles training sees (`ts=True`), so a
    cone is detected at the pixel size the model learnt it at instead of shrunk with the whole frame.  `scale`: a float, or a callable
    (frame_w, frame_h) -> float (the data set's scales are per camera size).  Boxes of overlapping tiles are merged by the greedy NMS at
    `nms_thres`; `contain_thres` (None: off) also removes a box of one tile that lies to more than that fraction of the smaller area
    inside a more confident box of another tile -- the part of a cone a tile edge cut off.  Yields `TiledFrameDetections` (boxes in
    frame pixels: merged box / scale).  ONE host synchronisation per batch."""

    _result_type = TiledFrameDetections

    def __init__(self, model, scale, conf_thres=None, nms_thres=None, top_k=200, max_boxes=200, outline=(255, 0, 0), batch_size=16,
                 tile_batch=32, contain_thres=None):
        super().__init__(model, conf_thres, nms_thres, top_k, max_boxes, outline, batch_size)
        self._init_tiles(scale, tile_batch, contain_thres)

    def _plan(self, sizes, first):
        return TiledBatchPlan(sizes, self.width, self.height, self.top_k, self._scales(sizes), first)


class TiledFrameConeDetector(_Tiled, FrameConeDetector):
    """`TiledFrameConeDetector(model, keypoint_net, scale)`: TiledFrameDetector's boxes carried through FrameConeDetector's crop ->
    key-point -> draw chain (the crops are cut from the untouched full-resolution frames in the pool).  Yields `TiledFrameCones`."""

    _result_type = TiledFrameCones

    def __init__(self, model, keypoint_net, scale, conf_thres=None, nms_thres=None, top_k=200, max_boxes=200, outline=(255, 0, 0),
                 batch_size=16, max_cones=64, bucket=64, colours=KPT_COLOURS_RGB, tile_batch=32, contain_thres=None):
        super().__init__(model, keypoint_net, conf_thres, nms_thres, top_k, max_boxes, outline, batch_size, max_cones, bucket, colours)
        self._init_tiles(scale, tile_batch, contain_thres)

    def _plan(self, sizes, first):
        return TiledConeBatchPlan(sizes, self.width, self.height, self.top_k, self._scales(sizes), self.max_cones, first)


# --------------------------------------------------------------------------------------------- the reference's two functions (detect.py)
def _open_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode != "RGB":
            raise ValueError(f"{path}: Pillow mode {im.mode!r} is not supported, only 'RGB' (the reference draws on the unconverted image, "
                             f"where the ink of outline=\"red\" depends on the mode); convert the file to RGB first")
        return np.asarray(im, dtype=np.uint8)


def _save(annotated, path):
    from PIL import Image
    Image.fromarray(annotated).save(path)
    return path


def _detector(model, device, conf_thres, nms_thres, tiles=False, scale=1.0, contain_thres=None, **kw):
    """`device` is where the reference moves its input (detect.py:78) and where the caller has put the model (detect.py:51): the batches
    are built on the model's device, so the two must be the same GPU.  None: the model's device.  `tiles`: a TiledFrameDetector at
    `scale` with `contain_thres`; otherwise those two are not looked at."""
    if device is not None:
        want, have = torch.device(device), next(model.parameters()).device
        if want.type != "cuda":
            raise _lib.MdcvError(f"detect: device {device!r} is not a GPU; there is no CPU fallback")
        if have.type != "cuda" or (want.index is not None and want.index != have.index):
            raise ValueError(f"detect: device {device!r} is not the model's device {str(have)!r}; move the model there first, as the reference's main does")
    if tiles:
        return TiledFrameDetector(model, scale, conf_thres=conf_thres, nms_thres=nms_thres, contain_thres=contain_thres, **kw)
    return FrameDetector(model, conf_thres=conf_thres, nms_thres=nms_thres, **kw)


def single_img_detect(target_path, output_path, mode, model, device, conf_thres, nms_thres, *, tiles=False, scale=1.0, contain_thres=None):
    """detect.py:60-111 for one RGB image file: mode 'image' saves under `output_path` with the file's own name, any other mode saves over
    `target_path` (the reference's rule for its dumped video frames); the saved path is returned.  With no detection the image is
    saved unannotated.  `device` must be the GPU the model is on (or None).  Each call builds its own detector: for many files use `detect`
    on their directory.  Keyword-only `tiles=True`: tile-and-scale inference at `scale` (TiledFrameDetector), the counterpart of training
    with ts=True; the defaults are the reference's whole-frame pad and resize."""
    frame = _open_rgb(target_path)
    res = next(iter(_detector(model, device, conf_thres, nms_thres, tiles, scale, contain_thres, batch_size=1).detect_frames([frame])))
    if mode == "image":
        return _save(res.annotated, os.path.join(output_path, target_path.split("/")[-1]))
    return _save(res.annotated, target_path)


def detect(target_path, output_path, model, device, conf_thres, nms_thres, batch_size=16, *, tiles=False, scale=1.0, contain_thres=None):
    """detect.py:113-196.  An image file (.jpg / .jpeg / .png / .tif) goes through `single_img_detect`; a directory has its image files,
    sorted by name, detected in batches of `batch_size` and written to `output_path` under their own names (-> the list of paths).
    Video containers need cv2 for decode and encode: ValueError; feed decoded frames to `FrameDetector.detect_frames` instead.
    Keyword-only `tiles`, `scale`, `contain_thres`: as in `single_img_detect`."""
    ext = os.path.splitext(target_path)[-1].lower()
    if os.path.isdir(target_path):
        names = sorted(f for f in os.listdir(target_path)
                       if os.path.splitext(f)[-1].lower() in IMG_FORMATS and os.path.isfile(os.path.join(target_path, f)))
        print(f"Detection Mode is: directory ({len(names)} images)")
        det = _detector(model, device, conf_thres, nms_thres, tiles, scale, contain_thres, batch_size=batch_size)
        frames = (_open_rgb(os.path.join(target_path, f)) for f in names)
        paths = [_save(res.annotated, os.path.join(output_path, f)) for f, res in zip(names, det.detect_frames(frames))]
        print(f"Please check output images at {output_path}")
        return paths
    if ext in VID_FORMATS:
        raise ValueError(f"{target_path}: video containers ({', '.join(VID_FORMATS)}) need cv2 to decode and encode, which this build does "
                         f"not use; decode the frames yourself and pass them to mdcv.yolo.detect.FrameDetector.detect_frames, or dump them "
                         f"to a directory and pass that")
    if ext not in IMG_FORMATS:
        raise ValueError(f"{target_path}: not an image file ({', '.join(IMG_FORMATS)}) or a directory")
    print("Detection Mode is: image")
    path = single_img_detect(target_path=target_path, output_path=output_path, mode="image", model=model, device=device,
                             conf_thres=conf_thres, nms_thres=nms_thres, tiles=tiles, scale=scale, contain_thres=contain_thres)
    print(f"Please check output image at {path}")
    return path
