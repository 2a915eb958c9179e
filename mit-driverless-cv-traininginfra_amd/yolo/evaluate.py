"""Dataset-level detection evaluation on the device: COCO-style average precision (csrc/detmap.hip).

`validate` reports the reference's figure, a mean of per-image APs at one IoU threshold.  `DatasetAP` computes the standard protocol
instead: ONE precision / recall curve per class over the whole validation set, at IoU 0.50:0.05:0.95, per range of box area, with
ignore regions.  Every `add*` call is one kernel launch with no synchronisation and no read-back (the image counter lives on the host);
`result()` sorts, walks the curves and reads back once.  The result is integer-exact up to the last step (101 fp64 divisions and additions
in a fixed order), so two runs -- or any split of the same images into batches -- give the same bits.

    ap = DatasetAP(num_classes=1, max_images=len(loader.dataset), area_ranges=((0, inf), (0, 32 ** 2), (32 ** 2, inf)))
    for _uris, imgs, targets in loader:
        det = detect_postprocess(model(imgs), targets, conf, nms, iou, width, height)
        ap.add(det, targets, width, height)
    r = ap.result();  r.AP, r.AP50, r.AP50_by_range

`python -m mdcv.yolo.evaluate --model_cfg ... --weights_path ...` evaluates the cfg's validation CSV; with `--frames DIR --labels CSV`
it scores whole frames (`--tiles --scale s`: through TiledFrameDetector) against the CSV's boxes in frame pixels.
"""
import math
import time

import numpy as np
import torch

from .. import _lib
from .postprocess import L_MAX_TOPK, detect_postprocess

COCO_IOU_THRESHOLDS = tuple(np.float32(0.5) + np.float32(0.05) * np.float32(i) for i in range(10))
MAX_GT, MAX_THR, MAX_RANGES, MAX_CLASSES, MAX_SLOTS = 2048, 10, 4, 1024, 1 << 30      # include/mdcv_hip.h MDCV_DETMAP_*
GT_PIXELS, GT_LABELS = 0, 1


def _nanmean(a, axis=None):
    a = np.asarray(a, np.float64)
    ok = ~np.isnan(a)
    n = ok.sum(axis=axis)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ok, a, 0.0).sum(axis=axis) / n                   # NaN where nothing is left to average


class APResult:
    """What `DatasetAP.result()` returns.  C classes, J IoU thresholds, S area ranges:
    ap [C,J,S] float64 (-1 where the class has no ground truth in the range), n_gt [C,S], tp [C,J,S] and detections [C,J,S] (the non-ignored
    ones), max_recall [C,J,S] (NaN without ground truth), q [C,J,S,101,2] int64 (the precision envelope at recall k / 100 as an exact
    fraction), precision [C,J,S,101] float64, n_images.  Means are over the classes that have ground truth in the range."""

    def __init__(self, ap, tot, q, thresholds, ranges, n_images):
        self.ap, self.q, self.n_images = ap, q, n_images
        self.iou_thresholds, self.area_ranges = thresholds, ranges
        self.n_gt, self.tp, self.detections = tot[:, 0, :, 0], tot[..., 1], tot[..., 2]
        self.precision = q[..., 0].astype(np.float64) / q[..., 1].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.max_recall = np.where(tot[..., 0] > 0, tot[..., 1] / tot[..., 0].astype(np.float64), np.nan)

    @property
    def ap_per_class(self):
        """[C,S]: the mean over the IoU thresholds; NaN where the class has no ground truth in the range"""
        return np.where(self.n_gt > 0, np.where(self.ap < 0, 0.0, self.ap).mean(axis=1), np.nan)

    def _at(self, thr):
        j = [i for i, t in enumerate(self.iou_thresholds) if np.float32(t) == np.float32(thr)]
        if not j:
            raise ValueError(f"IoU threshold {thr} was not evaluated (have {[float(t) for t in self.iou_thresholds]})")
        return j[0]

    @property
    def AP_by_range(self):
        return _nanmean(self.ap_per_class, axis=0)

    @property
    def AP50_by_range(self):
        return _nanmean(np.where(self.n_gt > 0, self.ap[:, self._at(0.5), :], np.nan), axis=0)

    @property
    def AP(self):
        """AP@[thresholds] over range 0 (conventionally everything)"""
        return float(self.AP_by_range[0])

    @property
    def AP50(self):
        return float(self.AP50_by_range[0])

    def summary(self):
        lo, hi = float(self.iou_thresholds[0]), float(self.iou_thresholds[-1])
        per = ", ".join(f"[{a:g}, {b:g}): {v:6.2%}" for (a, b), v in zip(self.area_ranges, self.AP50_by_range))
        head = f"AP@[{lo:.2f}:{hi:.2f}]" if len(self.iou_thresholds) > 1 else f"AP@{lo:.2f}"
        ap50 = f", AP50: {self.AP50:6.2%}" if any(np.float32(t) == np.float32(0.5) for t in self.iou_thresholds) else ""
        return f"{head}: {self.AP:6.2%}{ap50}, AP50 by area {per} ({self.n_images} images)"


class DatasetAP:
    """Accumulates detections and ground truth of up to `max_images` images on the device; see the module docstring.
    top_k: rows per image (the K of `detect_postprocess` / the detectors).  area_ranges: up to 4 [lo, hi) on box area in px^2."""

    def __init__(self, num_classes, max_images, top_k=200, iou_thresholds=COCO_IOU_THRESHOLDS, area_ranges=((0.0, math.inf),), device=None):
        self.C, self.cap, self.K = int(num_classes), int(max_images), int(top_k)
        self._thr = np.ascontiguousarray([np.float32(t) for t in iou_thresholds], np.float32)
        self._rng = np.ascontiguousarray(area_ranges, np.float32).reshape(-1, 2)
        self.J, self.S = len(self._thr), len(self._rng)
        if not 0 < self.K <= L_MAX_TOPK:
            raise ValueError(f"DatasetAP: top_k must be in 1..{L_MAX_TOPK}, got {top_k}")
        if not 1 <= self.C <= MAX_CLASSES or not 1 <= self.J <= MAX_THR or not 1 <= self.S <= MAX_RANGES:
            raise ValueError(f"DatasetAP: need 1..{MAX_CLASSES} classes, 1..{MAX_THR} IoU thresholds and 1..{MAX_RANGES} area ranges")
        if not 1 <= self.cap or self.cap * self.K > MAX_SLOTS:
            raise ValueError(f"DatasetAP: max_images * top_k must be in 1..{MAX_SLOTS}")
        if not ((self._thr > 0) & (self._thr <= 1)).all() or not (self._rng[:, 0] <= self._rng[:, 1]).all():
            raise ValueError("DatasetAP: IoU thresholds must lie in (0, 1] and every area range needs lo <= hi")
        self._device = device
        self.score = self.cls = self.count = self.status = self.n_gt = self._ws = None        # allocated by the first call that needs them
        self.n_images = 0

    def _alloc(self):
        if self.score is not None:
            return
        _lib.require_gpu()
        self.device = torch.device("cuda", torch.cuda.current_device()) if self._device is None else torch.device(self._device)
        dev, cap, K = self.device, self.cap, self.K
        self.score = torch.zeros(cap, K, dtype=torch.float32, device=dev)
        self.cls = torch.zeros(cap, K, dtype=torch.int32, device=dev)
        self.count = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.status = torch.zeros(self.S, cap, K, dtype=torch.int32, device=dev)            # two bits per threshold
        self.n_gt = torch.zeros(self.S, self.C, dtype=torch.int64, device=dev)

    def reset(self):
        """forget every image (one memset; nothing is read)"""
        if self.n_gt is not None:
            self.n_gt.zero_()
        self.n_images = 0

    # -- one launch: B images at slots n_images .. n_images + B - 1
    def _match(self, boxes, prob, cls, count, mode, gt, gt_cls, gt_ignore, gt_count, T, width, height):
        B = int(boxes.shape[0])
        if boxes.dim() != 3 or tuple(boxes.shape[1:]) != (self.K, 4) or tuple(prob.shape) != (B, self.K) or tuple(count.shape) != (B,):
            raise ValueError(f"DatasetAP: need boxes [B, {self.K}, 4], prob [B, {self.K}] and count [B]")
        if self.n_images + B > self.cap:
            raise ValueError(f"DatasetAP: {self.n_images} + {B} images exceed max_images = {self.cap}")
        if T > MAX_GT:
            raise ValueError(f"DatasetAP: at most {MAX_GT} ground-truth rows per image, got {T}")

        def dev(t, dtype, shape, what):
            if t is None:
                return None
            _lib.require_gpu(t)
            t = t.detach().to(dtype=dtype).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"DatasetAP: {what} must be {list(shape)}, got {list(t.shape)}")
            return t
        boxes, prob = dev(boxes, torch.float32, (B, self.K, 4), "boxes"), dev(prob, torch.float32, (B, self.K), "prob")
        cls, count = dev(cls, torch.int32, (B, self.K), "cls"), dev(count, torch.int32, (B,), "count")
        if T:
            gt = dev(gt, torch.float32, (B, T, 5 if mode == GT_LABELS else 4), "the ground truth")
            gt_cls, gt_count = dev(gt_cls, torch.int32, (B, T), "gt_cls"), dev(gt_count, torch.int32, (B,), "gt_count")
            gt_ignore = dev(gt_ignore, torch.uint8, (B, T), "gt_ignore")
        else:
            gt = gt_cls = gt_count = gt_ignore = None
        if B == 0:
            return
        self._alloc()
        p = lambda t: None if t is None else t.data_ptr()     # noqa: E731
        L = _lib.lib()
        with torch.cuda.device(self.device):
            L.check(L.detmap_match(p(boxes), p(prob), p(cls), p(count), B, self.K, mode, p(gt), p(gt_cls), p(gt_ignore), p(gt_count), T,
                                   float(width), float(height), self._thr.ctypes.data, self.J, self._rng.ctypes.data, self.S, self.C,
                                   self.n_images, self.cap, self.score.data_ptr(), self.cls.data_ptr(), self.count.data_ptr(),
                                   self.status.data_ptr(), self.n_gt.data_ptr(), torch.cuda.current_stream().cuda_stream), "detmap_match")
        self.n_images += B

    def add(self, det, targets, width, height):
        """det: the `Detections` of `detect_postprocess` for a batch; targets: the loader's zero-padded label rows [B,T,5] (or None)."""
        T = 0 if targets is None or targets.numel() == 0 else int(targets.shape[1])
        self._match(det.boxes, det.prob, det.cls, det.count, GT_LABELS, targets if T else None, None, None, None, T, width, height)

    def add_boxes(self, boxes, prob, cls, count, gt_boxes, gt_cls, gt_count, gt_ignore=None):
        """device tensors from anywhere: boxes [B,K,4] corner pixels, prob [B,K], cls [B,K] or None (class 0), count [B]; gt_boxes [B,T,4]
        corner pixels in the same coordinates, gt_cls [B,T] or None (class 0), gt_count [B], gt_ignore [B,T] or None."""
        T = 0 if gt_boxes is None or gt_boxes.numel() == 0 else int(gt_boxes.shape[1])
        self._match(boxes, prob, cls, count, GT_PIXELS, gt_boxes, gt_cls, gt_ignore, gt_count, T, 1.0, 1.0)

    @staticmethod
    def pack_frames(results, labels, K, scale=None, ignore=None):
        """the host half of `add_frames` -> boxes [B,K,4] f32, prob [B,K] f32, count [B] i32, gt [B,T,4] f32, gt_count [B] i32, gt_ignore
        [B,T] u8.  A frame with more than K boxes keeps the first K (they are most confident first)."""
        results, labels = list(results), [np.asarray(l, np.float64).reshape(-1, 4) for l in labels]
        if len(results) != len(labels) or (ignore is not None and len(ignore) != len(labels)):
            raise ValueError("add_frames: one label array (and one ignore array) per frame")
        B, T = len(results), max([len(l) for l in labels] + [1])
        boxes, prob, count = np.zeros((B, K, 4), np.float32), np.zeros((B, K), np.float32), np.zeros(B, np.int32)
        gt, gt_count, gt_ignore = np.zeros((B, T, 4), np.float32), np.zeros(B, np.int32), np.zeros((B, T), np.uint8)
        for b, (r, l) in enumerate(zip(results, labels)):
            n = min(len(r.boxes), K)
            boxes[b, :n], prob[b, :n], count[b] = np.asarray(r.boxes, np.float64)[:n], np.asarray(r.prob)[:n], n
            gt[b, :len(l)] = l if scale is None else l * float(scale)                     # float64 on the host, rounded once to float32
            gt_count[b] = len(l)
            if ignore is not None:
                gt_ignore[b, :len(l)] = np.asarray(ignore[b]).reshape(-1) != 0
        return boxes, prob, count, gt, gt_count, gt_ignore

    def add_frames(self, results, labels, scale=None, ignore=None):
        """results: `FrameDetections` / `TiledFrameDetections` of some frames; labels: per frame an [n,4] array of corner boxes
        (x0, y0, x1, y1) in the coordinates of the results' boxes -- frame pixels for FrameDetector, scaled-frame pixels for the tiled
        detectors, for which `scale=` multiplies the frame-pixel labels on the host (float64) before the upload.  ignore: per frame
        [n] flags.  Class 0.  Packed into one pinned buffer, one asynchronous copy, one launch."""
        arrays = self.pack_frames(results, labels, self.K, scale, ignore)
        if len(arrays[0]) == 0:
            return
        sizes = [(a.nbytes + 15) // 16 * 16 for a in arrays]
        self._alloc()
        pin = torch.empty(sum(sizes), dtype=torch.uint8).pin_memory()
        host, at = pin.numpy(), 0
        for a, n in zip(arrays, sizes):
            host[at:at + a.nbytes] = a.reshape(-1).view(np.uint8)
            at += n
        dbuf = pin.to(self.device, non_blocking=True)
        views, at = [], 0
        for a, n in zip(arrays, sizes):
            dt = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}[a.dtype]
            views.append(dbuf[at:at + a.nbytes].view(dt).view(a.shape))
            at += n
        boxes, prob, count, gt, gt_count, gt_ignore = views
        self.add_boxes(boxes, prob, None, count, gt, None, gt_count, gt_ignore)

    def result(self):
        """finalize and the evaluator's one read-back -> `APResult`"""
        L = _lib.lib()
        self._alloc()
        C, J, S = self.C, self.J, self.S
        n_ap, n_tot, n_q = C * J * S, C * J * S * 3, C * J * S * 101 * 2
        with torch.cuda.device(self.device):
            if self._ws is None:
                nbytes = int(L.detmap_finalize_workspace_bytes(self.cap, self.K))
                if nbytes < 0:
                    raise _lib.MdcvError(f"libmdcv_hip: detmap_finalize_workspace_bytes failed with code {nbytes}")
                self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            out = torch.empty(n_ap + n_tot + n_q + 1, dtype=torch.int64, device=self.device)
            base = out.data_ptr()
            L.check(L.detmap_finalize(self.score.data_ptr(), self.cls.data_ptr(), self.count.data_ptr(), self.status.data_ptr(),
                                      self.n_gt.data_ptr(), self.n_images, self.cap, self.K, J, S, C, base + 8 * (n_ap + n_tot),
                                      base + 8 * n_ap, base, base + 8 * (n_ap + n_tot + n_q), self._ws.data_ptr(), self._ws.numel(),
                                      torch.cuda.current_stream().cuda_stream), "detmap_finalize")
            host = out.cpu().numpy()
        if int(host[-1:].view(np.int32)[0]) & 1:
            raise _lib.MdcvError("DatasetAP: a valid detection has a NaN or non-positive score; scores must be > conf_thres > 0")
        ap = host[:n_ap].view(np.float64).reshape(C, J, S).copy()
        tot = host[n_ap:n_ap + n_tot].reshape(C, J, S, 3).copy()
        q = host[n_ap + n_tot:n_ap + n_tot + n_q].reshape(C, J, S, 101, 2).copy()
        return APResult(ap, tot, q, tuple(self._thr), [tuple(float(v) for v in r) for r in self._rng], self.n_images)


def evaluate(*, dataloader, model, device, step=-1, bbox_all=False, debug_mode=False, top_k=200, iou_thresholds=COCO_IOU_THRESHOLDS,
             area_ranges=((0.0, math.inf), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, math.inf))):
    """`validate`'s loop with a `DatasetAP` beside the per-image statistics: one more launch per batch, nothing more read per batch.
    -> ((mean_mAP, mean_R, mean_P, seconds_per_image) exactly as `validate` returns them, APResult).  Prints validate's line, then one
    line of AP@[.5:.95], AP50 and AP50 per area range (box areas in network-input px^2)."""
    with torch.no_grad():
        t_start = time.time()
        conf_thres, nms_thres, iou_thres = model.get_threshs()
        width, height = model.img_size()
        model.eval()
        n_images = len(dataloader.dataset)
        acc = DatasetAP(model.get_num_classes(), max(n_images, 1), top_k=top_k, iou_thresholds=iou_thresholds, area_ranges=area_ranges,
                        device=device)
        stats = []
        for _uris, imgs, targets in dataloader:
            imgs = imgs.to(device, non_blocking=True)
            targets = targets.to(device, non_blocking=True)
            det = detect_postprocess(model(imgs), targets, conf_thres, nms_thres, iou_thres, width, height, top_k)
            stats.append(det.stats)
            acc.add(det, targets, width, height)
        if stats:
            s = torch.cat(stats, 0)
            valid = s[:, 3] > 0
            n = int(valid.sum().item())
            means = (s[valid, :3].sum(0) / max(n, 1)).tolist() if n else [float("nan")] * 3
        else:
            means = [float("nan")] * 3
        res = acc.result()
        torch.cuda.synchronize()
        dt = time.time() - t_start
        mean_mAP, mean_R, mean_P = means
        print('mAP: {0:5.2%}, Recall: {1:5.2%}, Precision: {2:5.2%}'.format(mean_mAP, mean_R, mean_P))
        print(res.summary())
        return (mean_mAP, mean_R, mean_P, dt / (n_images + 1e-12)), res


def evaluate_frames(frames, labels, detector, scale=None, area_ranges=((0.0, math.inf),), iou_thresholds=COCO_IOU_THRESHOLDS, batch=64):
    """whole frames through a `FrameDetector` / `TiledFrameDetector` against per-frame corner boxes in frame pixels -> APResult.
    scale: the tiled detector's constant scale (its boxes are in scaled-frame pixels, so the labels are multiplied by it)."""
    labels = list(labels)
    acc = DatasetAP(1, max(len(labels), 1), top_k=detector.top_k, iou_thresholds=iou_thresholds, area_ranges=area_ranges, device=detector.device)
    pending = []
    for r in detector.detect_frames(frames):
        pending.append(r)
        if len(pending) == batch:
            acc.add_frames(pending, labels[acc.n_images:acc.n_images + batch], scale=scale)
            pending = []
    if pending:
        acc.add_frames(pending, labels[acc.n_images:acc.n_images + len(pending)], scale=scale)
    return acc.result()


def main(argv=None):
    import argparse
    import os
    from .models import Darknet
    p = argparse.ArgumentParser(description="COCO-style AP of a detector over its validation set, or over whole frames")
    p.add_argument('--model_cfg', type=str, required=True, help='cfg file path')
    p.add_argument('--weights_path', type=str, required=True, help='weights path')
    p.add_argument('--dataset_path', type=str, default="dataset/YOLO_Dataset/", help='path to image dataset')
    p.add_argument('--batch_size', type=int, default=16)
    p.add_argument('--no_ts', dest='ts', action='store_false', help='letterbox whole images instead of tiles (validation CSV mode)')
    p.add_argument('--frames', type=str, default=None, help='directory of whole frames: score frame-level detections')
    p.add_argument('--labels', type=str, default=None, help='CSV in the training layout naming the frames and their boxes')
    p.add_argument('--tiles', action='store_true', help='frame mode: tile-and-scale inference (TiledFrameDetector)')
    p.add_argument('--scale', type=float, default=1.0, help='frame mode with --tiles: the scale')
    p.add_argument('--contain_thres', type=float, default=None, help='frame mode with --tiles: the seam rule of the tile merge')
    p.add_argument('--conf_thres', type=float, default=None, help='frame mode: confidence threshold (default: the cfg\'s)')
    p.add_argument('--nms_thres', type=float, default=None, help='frame mode: NMS threshold (default: the cfg\'s)')
    p.add_argument('--precision', type=str, default=None, choices=["bf16", "fp32"], help='precision of the network (default: the model\'s)')
    a = p.parse_args(argv)
    device = torch.device("cuda", torch.cuda.current_device())
    model = Darknet(config_path=a.model_cfg, xy_loss=2, wh_loss=1.6, no_object_loss=25, object_loss=0.1, vanilla_anchor=False, precision=a.precision)
    model.load_weights(a.weights_path, model.get_start_weight_dim())
    model = model.to(device).eval()
    if (a.frames is None) != (a.labels is None):
        p.error("--frames and --labels go together")
    if a.frames is None:
        from ..data.images import ImageLabelBatches
        width, height = model.img_size()
        loader = ImageLabelBatches(model.get_links()[0], a.dataset_path, width, height, num_images=model.num_images()[0], bw=model.get_bw(),
                                   ts=a.ts, batch_size=a.batch_size, shuffle=False, device=device)
        return evaluate(dataloader=loader, model=model, device=device)[1]
    from ..data.images.labels import read_label_csv
    from .detect import _detector, _open_rgb
    rows = read_label_csv(a.labels, a.frames)
    labels = [np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 3], b[:, 1] + b[:, 2]], axis=1).astype(np.float64) for *_x, b in rows]   # (x, y, h, w)
    det = _detector(model, device, a.conf_thres, a.nms_thres, a.tiles, a.scale, a.contain_thres, batch_size=a.batch_size)
    frames = (_open_rgb(os.path.join(a.frames, os.path.basename(r[0]))) for r in rows)
    res = evaluate_frames(frames, labels, det, scale=a.scale if a.tiles else None,
                          area_ranges=((0.0, math.inf), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, math.inf)))
    print(res.summary())
    return res


if __name__ == "__main__":
    main()
