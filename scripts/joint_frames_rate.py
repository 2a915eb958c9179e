"""Frames and cones per second from decoded frames to annotated frames with key points (mdcv.yolo.detect.FrameConeDetector,
csrc/kpt_detect.hip) on one GPU, DESIGN 20.

yolo_baseline at 608 x 608 (bench.py's generated cfg, random weights re-drawn as scripts/detect_rate.py re-draws them, at the first
(trunk, head) gain whose boxes can be drawn, bf16), a random-weight
KeypointNet at 80 x 80 (bf16), N synthetic 1920 x 1200 RGB frames already decoded in host memory, batch_size 16.  The confidence threshold
is taken from the model's own objectness on the first frames so that about 40 candidates per frame pass it; the calibration is printed.  Two paths, each warmed up,
alternated in one run, host clock around work that ends in a synchronise:

(a) the same work chained from the earlier public pieces: FrameDetector.detect_frames (boxes mapped and outlined on the device, frames
    copied back), then per frame on the host the rect windows cut out of the ORIGINAL frame, ConeCropBatches' transform_batch (upload and
    the 8-bit resize), one KeypointNet eval per frame's crops, the key points read back, and a host draw of the discs (NumPy stores)
(b) FrameConeDetector.detect_frames, batch_size 16

Both print frames/s and cones/s (boxes with a crop).  No ratio is required of anyone; the numbers go into DESIGN 20 with the command.

usage: joint_frames_rate.py [frames (default 64)] [rounds (default 3)]"""
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from mdcv.data import crops as CR  # noqa: E402
from mdcv.data import images as I  # noqa: E402
from mdcv.rektnet.keypoint_net import KeypointNet  # noqa: E402
from mdcv.yolo.detect import KPT_COLOURS_RGB, FrameConeDetector, FrameDetector  # noqa: E402
from mdcv.yolo.models import Darknet  # noqa: E402

FW, FH, SIDE, BATCH, MAX_CONES, BUCKET = 1920, 1200, 608, 16, 64, 64
DISC = [(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3) if abs(dx) + abs(dy) <= 2]
LABEL = np.zeros((7, 2))                           # transform_batch wants labels; the heat-maps they give are not used


def make_model(trunk_gain, head_gain):
    with tempfile.TemporaryDirectory(prefix="joint_rate_") as workdir:
        cfg = bench.write_yolo_cfg(workdir, SIDE, 80)
        cwd = os.getcwd()
        os.chdir(workdir)
        try:
            torch.manual_seed(0)
            net = Darknet(cfg, 2.0, 1.6, 25.0, 0.1, True, precision="bf16")
        finally:
            os.chdir(cwd)
    with torch.no_grad():                # see scripts/detect_rate.py: every convolution re-drawn at `trunk_gain`, the three heads at `head_gain`
        for index, layer in enumerate(net.module_defs):
            head = index + 1 < len(net.module_defs) and net.module_defs[index + 1]["type"] == "yolo"
            for p in net.module_list[index].parameters():
                if p.dim() == 4:
                    fan_in = p.shape[1] * p.shape[2] * p.shape[3]
                    p.normal_(0.0, (head_gain if head else trunk_gain) / fan_in ** 0.5)
    return net.cuda().eval()


def threshold(model, frames):
    geoms = [I.sample_geometry(FW, FH, SIDE, SIDE, ts=False) for _ in range(4)]
    with torch.no_grad():
        obj = model(I.transform_batch(frames[:4], geoms))[..., 4].float()
    top = torch.sort(obj, dim=1, descending=True)[0]
    conf = float(top[:, 40].min())
    if float(top[:, 0].min()) <= conf:
        below = obj[obj < conf]
        if below.numel() == 0:
            return None
        conf = float(below.max())
    return conf


def calibrate(frames):
    """A model, built afresh per trial so that no launch plan holds earlier weights, at the first (trunk, head) gain and threshold at which
    the first frames keep boxes that can be drawn and cropped.  On an MI355X the gains of scripts/detect_rate.py (trunk 2 ** 0.5) saturate
    objectness at 1.0 at 608 x 608 for every head gain, and the one box kept per frame overflows: nothing to crop.  The smaller trunk
    gains are tried for that reason and have NOT been run yet.  -> (model, gain, conf)"""
    for gain in [(t, h) for t in (2.0 ** 0.5, 1.0, 0.7) for h in (4.0, 1.0, 0.25)]:
        model = make_model(*gain)
        conf = threshold(model, frames)
        if conf is None:
            continue
        res = list(FrameDetector(model, conf_thres=conf, batch_size=4).detect_frames(frames[:4]))
        drawable = sum(int((r.rects[:, 2] >= 0).sum()) for r in res) / 4
        print(f"    (trunk, head) gain {gain}: conf_thres {conf:.6f}, boxes kept {[len(r.boxes) for r in res]}, drawable per frame {drawable:.1f}")
        if drawable >= 10:
            return model, gain, conf
    raise SystemExit("no (trunk, head) gain gives boxes that can be drawn: nothing to measure")


def make_frames(n):
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (FH, FW, 3), dtype=np.uint8)
    return [np.roll(base, 37 * i, axis=1).copy() for i in range(n)]


def window(rect):
    x0, y0, x1, y1 = (int(v) for v in rect)
    cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x1, FW - 1), min(y1, FH - 1)
    if cx1 < cx0 or cy1 < cy0 or cx1 - cx0 >= CR.MAX_SIDE or cy1 - cy0 >= CR.MAX_SIDE:
        return None
    return cx0, cy0, cx1 - cx0 + 1, cy1 - cy0 + 1


def chained(det, kpnet, frames):
    """path (a) -> cones"""
    cones = 0
    for frame, res in zip(frames, det.detect_frames(frames)):
        wins = [w for w in (window(r) for r in res.rects[:MAX_CONES]) if w is not None]
        if not wins:
            continue
        cut = [np.ascontiguousarray(frame[y:y + h, x:x + w]) for x, y, w, h in wins]
        imgs, _, _ = CR.transform_batch(cut, [LABEL] * len(cut), 80)
        rows = (len(cut) + BUCKET - 1) // BUCKET * BUCKET
        batch = torch.zeros(rows, 3, 80, 80, device=imgs.device)
        batch[:len(cut)] = imgs
        with torch.no_grad():
            pts = kpnet(batch)[1][:len(cut)].cpu().numpy()
        out = res.annotated
        for (x, y, w, h), kp in zip(wins, pts):
            for i in range(7):
                cx, cy = x + int(np.float64(kp[i, 0]) * w), y + int(np.float64(kp[i, 1]) * h)
                for dx, dy in DISC:
                    if 0 <= cx + dx < FW and 0 <= cy + dy < FH:
                        out[cy + dy, cx + dx] = KPT_COLOURS_RGB[i]
        cones += len(cut)
    return cones


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def rates(n, rounds):
    frames = make_frames(n)
    torch.manual_seed(1)
    kpnet = KeypointNet(7, (80, 80), precision="bf16").cuda().eval()
    model, gain, conf = calibrate(frames)
    nms_thres = model.get_threshs()[1]
    plain = FrameDetector(model, conf_thres=conf, nms_thres=nms_thres, batch_size=BATCH)
    joint = FrameConeDetector(model, kpnet, conf_thres=conf, nms_thres=nms_thres, batch_size=BATCH, max_cones=MAX_CONES, bucket=BUCKET)
    paths = {"a": lambda: chained(plain, kpnet, frames),
             "b": lambda: sum(int(r.has_crop.sum()) for r in joint.detect_frames(frames))}
    res = {k: fn() for k, fn in paths.items()}                                    # warm-up: plans, pinned buffers
    t = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            t[k].append(timed(fn)[0])
    print(f"yolo_baseline {SIDE}x{SIDE} bf16 ((trunk, head) gain {gain}) + KeypointNet 80x80 bf16, {n} frames of {FW}x{FH}, conf_thres {conf:.4f}, nms_thres {nms_thres}, "
          f"{rounds} alternated rounds (frames/s per round; median)")
    what = {"a": "chained public pieces, host crops and draw", "b": f"FrameConeDetector, batches of {BATCH}         "}
    for k in paths:
        r = sorted(n / v for v in t[k])
        med = r[len(r) // 2]
        print(f"    ({k}) {what[k]} " + " / ".join(f"{n / v:8.1f}" for v in t[k]) + f"   median {med:8.1f} frames/s, {med * res[k] / n:9.1f} cones/s"
              f"   ({res[k]} cones in {n} frames)")


if __name__ == "__main__":
    torch.cuda.set_device(0)
    rates(int(sys.argv[1]) if len(sys.argv) > 1 else 64, int(sys.argv[2]) if len(sys.argv) > 2 else 3)
