"""Key points of cone crops, drawn on the device: the native counterpart of RektNet/detect.py for files and for batches.

The reference's `main` (detect.py:13-55) costs, per crop file, a cv2 resize on the host, a batch-1 forward on the CPU, seven host
normalisations of the heat-maps (:40-47) and seven `cv2.circle` calls (utils.py:61-66).  `KeypointDetector.detect_crops` runs the same
steps over batches of decoded crops of any sizes that stay on the device from the upload to the two pictures:

  1. the crops of a batch are packed into one pinned buffer at 16-byte-aligned offsets behind their descriptors; one H2D copy; each crop
     is its own image of the batch's pool (the `MDCV_DETECT_DESC` table of mdcv.yolo.detect, ratio 1, no pads),
  2. `mdcv_crop_resize_frames_u8` with one whole-image rect per crop: cv2's 8-bit resize to S x S and `/ 255.0`, planes B, G, R,
  3. `model.eval()`, forward under `no_grad` -> heat-maps and key points,
  4. `mdcv_kpt_draw_points`: each key point as `cv2.circle(img, (int(x * w), int(y * h)), 2, colour, -1)` into the crop in the pool,
  5. `mdcv_kpt_heatmap_mosaic`: the seven normalised heat-maps stacked into one 8-bit picture,
  6. one D2H copy,

with ONE host synchronisation per batch.  `detect` takes the reference's argument list for a file, so a caller swaps the import
(INTEGRATION.md); it also accepts a directory.  Departures, all in DESIGN.md §20: a constant heat-map gives zeros (the reference divides by
zero); a key point that is not finite is not drawn and counted; files are read and written with Pillow (RGB in memory; the colour table is
the reference's BGR table reversed, so the picture is the same); `flip` and `rotate` are accepted and ignored, as in the reference.
"""
import os
from itertools import islice

import numpy as np
import torch

from .. import _lib
from ..data.staging import align as _align, copy_back, pinned, upload
from ..yolo.detect import DETECT_DESC, IMG_FORMATS, KPT_COLOURS_RGB, NUM_KPT, _check_frame, _open_rgb, _save, colour_table, frame_offsets

MIN_SIZE, MAX_SIZE, MAX_SIDE = 16, 256, 4096          # MDCV_KPTLOAD_MIN_SIZE / MAX_SIZE / MAX_SIDE
_ONE = int(np.array([1.0], np.float64).view(np.int64)[0])


# ------------------------------------------------------------------------------------------------------------- host layout (no GPU)
class CropBatchPlan:
    """Byte layout of one batch of crops [(W, H)].  Device buffer: [descriptors B,6 i64] [rects B,1,4 i32] [count B i32] [pool: the
    crops] [keypoints B,7,2 f32] [centers B,7,2 i32] [skipped B i32] [owner B,2 i32] [window B,4 i32] [total 1 i32] [mosaic B,7S,S u8];
    the pinned input is everything up to the end of the pool, the copy back is everything from the pool on."""

    def __init__(self, sizes, S):
        B = len(sizes)
        self.B, self.S, self.sizes = B, int(S), [(int(w), int(h)) for w, h in sizes]
        for i, (w, h) in enumerate(self.sizes):
            if w > MAX_SIDE or h > MAX_SIDE:
                raise ValueError(f"detect_crops: crop {i} is {h}x{w} (h x w), over the resize kernel's bound of {MAX_SIDE} px a side")
        self.offsets, self.pool_bytes = frame_offsets(self.sizes)
        self.desc = np.zeros((B, DETECT_DESC), np.int64)
        self.rects = np.zeros((B, 4), np.int32)
        for b, ((w, h), off) in enumerate(zip(self.sizes, self.offsets)):
            self.desc[b] = off, w, h, _ONE, 0, 0
            self.rects[b] = 0, 0, w - 1, h - 1                              # the whole image: window (0, 0, w, h)
        self.desc_off = 0
        self.rect_off = _align(B * DETECT_DESC * 8)
        self.count_off = self.rect_off + B * 16
        self.pool_off = _align(self.count_off + B * 4)
        self.in_bytes = self.pool_off + self.pool_bytes
        self.pts_off = self.in_bytes
        self.centers_off = _align(self.pts_off + B * NUM_KPT * 8)
        self.skip_off = _align(self.centers_off + B * NUM_KPT * 8)
        self.owner_off = _align(self.skip_off + B * 4)
        self.window_off = _align(self.owner_off + B * 8)
        self.total_off = self.window_off + B * 16
        self.mosaic_off = self.total_off + 16
        self.nbytes = _align(self.mosaic_off + B * NUM_KPT * self.S * self.S)

    def pack(self, host, crops):
        """fill the pinned input (uint8 numpy, >= in_bytes) with the batch"""
        host[self.desc_off:self.desc_off + self.desc.nbytes].view(np.int64)[:] = self.desc.reshape(-1)
        host[self.rect_off:self.rect_off + self.rects.nbytes].view(np.int32)[:] = self.rects.reshape(-1)
        host[self.count_off:self.count_off + self.B * 4].view(np.int32)[:] = 1
        for c, off, (w, h) in zip(crops, self.offsets, self.sizes):
            host[self.pool_off + off:self.pool_off + off + 3 * w * h] = c.reshape(-1)


def image_name(path):
    """RektNet/detect.py:25"""
    return "_".join(path.split("/")[-1].split(".")[0].split("_")[-5:])


class KeypointDetector:
    """`KeypointDetector(model, img_size=80).detect_crops(crops)`: see the module docstring.  `model`: a KeypointNet on a GPU, built for
    `img_size`; `colours`: seven RGB triples, key point 0 to 6 (default: the reference's)."""

    def __init__(self, model, img_size=80, batch_size=16, colours=KPT_COLOURS_RGB):
        self.model, self.size, self.batch_size = model, int(img_size), int(batch_size)
        if not MIN_SIZE <= self.size <= MAX_SIZE:
            raise ValueError(f"KeypointDetector: img_size {img_size} outside {MIN_SIZE}..{MAX_SIZE}")
        if tuple(int(v) for v in model.image_size) != (self.size, self.size):
            raise ValueError(f"KeypointDetector: the model was built for image_size={tuple(model.image_size)}, not {(self.size, self.size)}")
        if int(getattr(model, "num_kpt", NUM_KPT)) != NUM_KPT:
            raise ValueError(f"KeypointDetector: the drawing kernel takes {NUM_KPT} key points per crop")
        if self.batch_size < 1:
            raise ValueError(f"KeypointDetector: batch_size must be positive, got {batch_size}")
        self.colours = colour_table(colours)
        self._pin_in = self._pin_out = None

    @property
    def device(self):
        return next(self.model.parameters()).device

    def _run(self, crops):
        L = _lib.lib()
        dev = self.device
        plan = CropBatchPlan([(c.shape[1], c.shape[0]) for c in crops], self.size)
        B, S = plan.B, plan.S
        self._pin_in = pinned(self._pin_in, plan.in_bytes)
        host = self._pin_in.numpy()
        plan.pack(host, crops)
        with torch.cuda.device(dev), torch.no_grad():
            st = torch.cuda.current_stream(dev)
            dbuf = upload(self._pin_in, plan.in_bytes, plan.nbytes, dev)
            base = dbuf.data_ptr()
            desc_h, desc_d = host.ctypes.data + plan.desc_off, base + plan.desc_off
            imgs = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
            L.check(L.crop_resize_frames_u8(desc_h, desc_d, B, base + plan.pool_off, plan.pool_bytes, base + plan.rect_off, base + plan.count_off,
                                            1, 1, S, imgs.data_ptr(), base + plan.owner_off, base + plan.window_off, base + plan.total_off,
                                            st.cuda_stream), "crop_resize_frames_u8")
            self.model.eval()
            hm, pts = self.model(imgs)
            if tuple(hm.shape) != (B, NUM_KPT, S, S):
                raise _lib.MdcvError(f"KeypointDetector: heat-maps of shape {tuple(hm.shape)}, expected {(B, NUM_KPT, S, S)}")
            hm = hm.contiguous()
            dbuf[plan.pts_off:plan.pts_off + B * NUM_KPT * 8].view(torch.float32).copy_(pts.reshape(-1))
            L.check(L.kpt_draw_points(desc_h, desc_d, B, base + plan.pool_off, plan.pool_bytes, base + plan.pts_off, base + plan.window_off,
                                      base + plan.owner_off, B, self.colours.ctypes.data, base + plan.centers_off, base + plan.skip_off,
                                      st.cuda_stream), "kpt_draw_points")
            L.check(L.kpt_heatmap_mosaic(hm.data_ptr(), B, S, base + plan.mosaic_off, st.cuda_stream), "kpt_heatmap_mosaic")
            self._pin_out, table = copy_back(dbuf, plan.pool_off, self._pin_out, st)      # the batch's one host synchronisation
        if int(table(plan.total_off, 4, np.int32, (1,))[0]) != B:
            raise _lib.MdcvError("KeypointDetector: the resize kernel refused a crop the host had accepted")
        kpts = table(plan.pts_off, B * NUM_KPT * 8, np.float32, (B, NUM_KPT, 2)).copy()       # the pinned buffer is the next batch's
        centers = table(plan.centers_off, B * NUM_KPT * 8, np.int32, (B, NUM_KPT, 2)).copy()
        mosaic = table(plan.mosaic_off, B * NUM_KPT * S * S, np.uint8, (B, NUM_KPT * S, S)).copy()
        for b, (off, (w, h)) in enumerate(zip(plan.offsets, plan.sizes)):
            yield kpts[b], centers[b], table(plan.pool_off + off, 3 * w * h, np.uint8, (h, w, 3)).copy(), mosaic[b]

    def detect_crops(self, crops):
        """crops: any iterable of (H, W, 3) uint8 RGB arrays (sizes may differ) -> yields, per crop and in order, (keypoints float32 [7,2]
        normalised x, y; centers int32 [7,2] as drawn, (-1, -1) for a point not drawn; annotated (H, W, 3) uint8; mosaic (7*S, S) uint8)"""
        _lib.require_gpu()
        it, first = iter(crops), 0
        while True:
            batch = [_check_frame(c, first + i) for i, c in enumerate(islice(it, self.batch_size))]
            if not batch:
                return
            first += len(batch)
            yield from self._run(batch)


# ------------------------------------------------------------------------------------------------- the reference's function (detect.py)
def load_model(model, img_size=80, device="cuda"):
    """`model`: a KeypointNet, or the path of a checkpoint read as detect.py:36-37 reads it (`torch.load(path).get('model')`)"""
    from .keypoint_net import KeypointNet
    if not isinstance(model, (str, os.PathLike)):
        return model
    net = KeypointNet(NUM_KPT, (int(img_size), int(img_size)))
    net.load_state_dict(torch.load(model, map_location="cpu").get("model"))
    return net.to(device).eval()


def detect(model, img, img_size=80, output="outputs/visualization/", flip=False, rotate=False, batch_size=16, ext=".jpg"):
    """RektNet/detect.py:13-55 (`main`).  `img`: an image file, or a directory whose image files (.jpg / .jpeg / .png / .tif), sorted by
    name, are run in batches of `batch_size`.  Per file it writes `output + <name> + "_hm" + ext` (the heat-map mosaic) and
    `output + <name> + "_inference" + ext` (the crop with its key points), `<name>` as detect.py:25 builds it and `output` joined as the
    reference joins it (plain concatenation for `_hm`; the directory must exist) -> the list of (inference path, hm path).  `flip` and
    `rotate` are accepted and ignored, as in the reference.  `ext`: ".png" for a lossless copy of the arrays."""
    if os.path.isdir(img):
        files = sorted(os.path.join(img, f) for f in os.listdir(img)
                       if os.path.splitext(f)[-1].lower() in IMG_FORMATS and os.path.isfile(os.path.join(img, f)))
    else:
        files = [img]
    det = KeypointDetector(load_model(model, img_size), img_size=img_size, batch_size=batch_size)
    paths = []
    for f, (_kp, _c, annotated, mosaic) in zip(files, det.detect_crops(_open_rgb(f) for f in files)):
        name = image_name(f)
        hm_path = _save(mosaic, output + name + "_hm" + ext)
        print(f"please check the output image here: {hm_path}")
        paths.append((_save(annotated, os.path.join(output, name + "_inference" + ext)), hm_path))
    return paths
