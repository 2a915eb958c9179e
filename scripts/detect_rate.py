"""Frames per second of batched detection (mdcv.yolo.detect.FrameDetector.detect_frames, csrc/detect_draw.hip) on one GPU, DESIGN 19.

yolo_baseline at 416 x 416 (bench.py's generated cfg, random weights re-drawn at a scale-preserving gain, the three head convolutions wider, bf16), N synthetic 1920 x 1200 RGB frames already decoded in host
memory, batch_size 16.  The confidence threshold is taken from the model's own objectness on the first frames so that about 40 candidates
per frame pass it.  Paths, each warmed up, alternated in one run, host clock around work that ends in a synchronise:

(a) the reference's per-frame procedure (CVC-YOLOv3/detect.py:60-104, restated below in this project's words, with its line numbers) on the same drop-in model:
    Pillow pad and resize, batch-1 forward, the confidence filter and utils.nms, four .item() per box, ImageDraw.  It starts from the
    decoded frame: the reference's JPEG write and re-read per video frame (detect.py:155, :62, :95) are NOT included, nor is its save.
(b) detect_frames, batch_size 16
(c) detect_frames, batch_size 16, keep_on_device=True (no D2H copy of pixels)

`draw`: mdcv_detect_draw_boxes alone, B = 16 frames of 1920 x 1200, K = 200, `per` boxes kept per frame, device events around back-to-back
launches, against its byte floor: the outline bytes written plus the tables read and written, over the copy rate given in TB/s.

usage: detect_rate.py [frames (default 64)] [rounds (default 3)]   |   detect_rate.py draw [boxes per frame (default 40)] [TB/s (default 5.2)]"""
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from mdcv import _lib  # noqa: E402
from mdcv.data import images as I  # noqa: E402
from mdcv.data.images import letterbox  # noqa: E402
from mdcv.yolo.detect import FrameDetector  # noqa: E402
from mdcv.yolo.models import Darknet  # noqa: E402
from mdcv.yolo.utils.nms import nms  # noqa: E402

FW, FH, BATCH = 1920, 1200, 16


def make_model():
    with tempfile.TemporaryDirectory(prefix="detect_rate_") as workdir:
        cfg = bench.write_yolo_cfg(workdir, 416, 80)
        cwd = os.getcwd()
        os.chdir(workdir)
        try:
            torch.manual_seed(0)
            net = Darknet(cfg, 2.0, 1.6, 25.0, 0.1, True, precision="bf16")
        finally:
            os.chdir(cwd)
    with torch.no_grad():                # as initialised (N(0, 0.02) weights, BatchNorm running statistics 0 / 1) the signal dies out on the
        for index, layer in enumerate(net.module_defs):     # way to the heads and objectness is one value everywhere: re-draw every
            head = index + 1 < len(net.module_defs) and net.module_defs[index + 1]["type"] == "yolo"      # convolution at a gain that
            for p in net.module_list[index].parameters():   # keeps the activations' scale, and the three heads wider, so that a
                if p.dim() == 4:                            # threshold can select boxes
                    fan_in = p.shape[1] * p.shape[2] * p.shape[3]
                    p.normal_(0.0, (4.0 if head else 2.0 ** 0.5) / fan_in ** 0.5)
    return net.cuda().eval()


def make_frames(n):
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (FH, FW, 3), dtype=np.uint8)
    return [np.roll(base, 37 * i, axis=1).copy() for i in range(n)]


def reference_frame(model, frame, conf_thres, nms_thres):
    """What single_img_detect (CVC-YOLOv3/detect.py:60-104) costs per frame, from the decoded frame to the annotated image, restated with
    the same operations in the same order: the comments cite the reference lines each step stands for.  torchvision's pad / resize /
    to_tensor are the Pillow and NumPy calls they wrap."""
    from PIL import Image, ImageDraw, ImageOps
    picture = Image.fromarray(frame)                                              # detect.py:62 (the decoded frame instead of a file)
    net_w, net_h = model.img_size()                                               # :64
    pad_w, pad_h, ratio = letterbox(picture.width, picture.height, net_w, net_h)  # :65 calculate_padding
    padded = ImageOps.expand(picture, border=(pad_w, pad_h, pad_w, pad_h), fill=(127, 127, 127))   # :66 F.pad
    small = padded.resize((net_w, net_h), Image.BILINEAR)                         # :67 F.resize
    chw = np.asarray(small, dtype=np.uint8).transpose(2, 0, 1).copy()
    batch = (torch.from_numpy(chw).float() / 255)[None]                           # :73-74 to_tensor, batch of one
    kept = None
    with torch.no_grad():                                                         # :76
        model.eval()                                                              # :77
        pred = model(batch.to("cuda", non_blocking=True))                         # :78-80 batch-1 forward
        for rows in pred:                                                         # :83 one image
            rows = rows[rows[:, 4] > conf_thres]                                  # :84 confidence mask
            half = rows[:, 2:4] / 2                                               # :87
            corners = torch.zeros((rows.shape[0], 4), device=rows.device)         # :85 a fresh corner tensor, filled in halves
            corners[:, :2] = rows[:, :2] - half                                   # :88
            corners[:, 2:] = rows[:, :2] + half                                   # :89
            kept = corners[nms(corners, rows[:, 4], nms_thres)]                   # :90-92 greedy NMS, one host read of the count
    canvas = Image.fromarray(frame)                                               # :95 a second image to draw on
    pen = ImageDraw.Draw(canvas)                                                  # :96
    for box in kept:                                                              # :99 per kept box:
        left, top, right, bottom = (box[j].to("cpu").item() for j in range(4))    # :100-103 four device reads
        pen.rectangle((left / ratio - pad_w, top / ratio - pad_h, right / ratio - pad_w, bottom / ratio - pad_h), outline="red")   # :100-104
    return canvas, len(kept)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def rates(n, rounds):
    model, frames = make_model(), make_frames(n)
    geoms = [I.sample_geometry(FW, FH, 416, 416, ts=False) for _ in range(4)]
    with torch.no_grad():
        obj = model(I.transform_batch(frames[:4], geoms))[..., 4].float()
    top = torch.sort(obj, dim=1, descending=True)[0]
    conf = float(top[:, 40].min())
    if float(top[:, 0].min()) <= conf:                                            # the 41 highest of a frame are one (saturated) value:
        below = obj[obj < conf]                                                   # step under it, so that `> conf` selects them
        assert below.numel() > 0, "the objectness is one value everywhere: no threshold selects boxes"
        conf = float(below.max())
    nms_thres = model.get_threshs()[1]
    det = FrameDetector(model, conf_thres=conf, nms_thres=nms_thres, batch_size=BATCH)
    paths = {"a": lambda: [reference_frame(model, f, conf, nms_thres)[1] for f in frames],
             "b": lambda: [len(r.boxes) for r in det.detect_frames(frames)],
             "c": lambda: [len(r.boxes) for r in det.detect_frames(frames, keep_on_device=True)]}
    res = {k: fn() for k, fn in paths.items()}                                    # warm-up: plans, pinned buffers
    t = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            t[k].append(timed(fn)[0])
    print(f"yolo_baseline 416x416 bf16, {n} frames of {FW}x{FH}, conf_thres {conf:.4f}, nms_thres {nms_thres}, {rounds} alternated rounds (frames/s per round; median)")
    what = {"a": "reference per-frame procedure   ", "b": f"detect_frames, batches of {BATCH}   ", "c": "the same, keep_on_device       "}
    med = {}
    for k in paths:
        r = sorted(n / v for v in t[k])
        med[k] = r[len(r) // 2]
        print(f"    ({k}) {what[k]} " + " / ".join(f"{n / v:8.1f}" for v in t[k]) + f"   median {med[k]:8.1f} frames/s ({1e3 / med[k]:7.2f} ms per frame)"
              f"   boxes kept {sum(res[k])}")
    print(f"    (b) / (a) = {med['b'] / med['a']:.2f}x   (c) / (a) = {med['c'] / med['a']:.2f}x")
    mb = 3 * FW * FH / 1e6
    print(f"    a frame is {mb:.2f} MB: (b) moves it over the host link twice, (c) once")


def draw(per, tbs):
    L = _lib.lib()
    B, K = BATCH, 200
    rng = np.random.default_rng(1)
    pad_w, pad_h, ratio = letterbox(FW, FH, 416, 416)
    offs = [b * ((3 * FW * FH + 15) // 16 * 16) for b in range(B)]
    pool = torch.zeros(offs[-1] + 3 * FW * FH, dtype=torch.uint8, device="cuda")
    desc = np.array([[o, FW, FH, np.array([ratio]).view(np.int64)[0], pad_w, pad_h] for o in offs], np.int64)
    cx, cy = rng.uniform(40, 376, (B, K)), rng.uniform(110, 300, (B, K))
    bw, bh = rng.uniform(4, 40, (B, K)), rng.uniform(6, 60, (B, K))
    boxes = np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], -1).astype(np.float32)
    count = np.full(B, per, np.int32)
    d_desc, d_boxes, d_count = torch.from_numpy(desc).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(count).cuda()
    fb = torch.empty(B, K, 4, dtype=torch.float64, device="cuda")
    rects = torch.empty(B, K, 4, dtype=torch.int32, device="cuda")
    skipped = torch.empty(B, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def run():
        L.check(L.detect_draw_boxes(desc.ctypes.data, d_desc.data_ptr(), B, d_boxes.data_ptr(), d_count.data_ptr(), K, pool.data_ptr(), pool.numel(),
                                    255, 0, 0, fb.data_ptr(), rects.data_ptr(), skipped.data_ptr(), st), "detect_draw_boxes")
    run()
    torch.cuda.synchronize()
    r = rects.cpu().numpy()[:, :per].astype(np.int64)
    x0, y0, x1, y1 = (np.clip(r[..., 0], 0, FW - 1), np.clip(r[..., 1], 0, FH - 1), np.clip(r[..., 2], 0, FW - 1), np.clip(r[..., 3], 0, FH - 1))
    outline = int((3 * (2 * (x1 - x0 + 1) + 2 * (y1 - y0))).sum())               # boxes inside the frame: two rows, two columns between them
    tables = B * per * (16 + 32 + 16) + B * (4 + 4 + 48)
    iters = 200
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        run()
    e.record()
    e.synchronize()
    us = 1e3 * s.elapsed_time(e) / iters
    floor = (outline + tables) / (tbs * 1e6)
    print(f"mdcv_detect_draw_boxes B={B} K={K}, {per} boxes per frame on {FW}x{FH}: {outline} outline bytes + {tables} table bytes, byte floor "
          f"{floor:.3f} us at {tbs} TB/s; back-to-back launches (events, memset included): {us:.2f} us = {us / floor:.0f} x floor "
          f"(grid {K} x {B} = {K * B} workgroups, {B * per} of them draw)")


if __name__ == "__main__":
    torch.cuda.set_device(0)
    if len(sys.argv) > 1 and sys.argv[1] == "draw":
        draw(int(sys.argv[2]) if len(sys.argv) > 2 else 40, float(sys.argv[3]) if len(sys.argv) > 3 else 5.2)
    else:
        rates(int(sys.argv[1]) if len(sys.argv) > 1 else 64, int(sys.argv[2]) if len(sys.argv) > 2 else 3)
