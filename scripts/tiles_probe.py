"""Tile-and-scale inference on one GPU, DESIGN 22: what it costs beside whole-frame detection, and what the merge launch costs.

`rates` (default): yolo_baseline at 416 x 416 (scripts/detect_rate.py's model: bench.py's generated cfg, weights re-drawn so that a threshold
selects boxes, bf16), N synthetic 1920 x 1200 RGB frames already decoded in host memory, batch_size 16.  Paths, each warmed up, alternated
in one run, host clock around work that ends in a synchronise:
    (w) FrameDetector.detect_frames: the whole frame padded and resized to 416 x 416, ONE network input per frame
    (t) TiledFrameDetector.detect_frames at scale 1.0: 15 tiles of 416 x 416 per frame, tile_batch 32, one mdcv_detect_merge_tiles per batch
    (s) the same with the seam rule on (contain_thres 0.6)
The confidence threshold is detect_rate.py's (about 40 candidates per whole frame pass it); both detectors use it.

`merge`: mdcv_detect_merge_tiles alone, B = 16 frames x 15 tiles, K = top_k = 200, `per` candidates per tile (random boxes over a 5 x 3 grid of
overlapping tiles), device events around back-to-back launches; beside it the same merge assembled from the pieces the tree had before:
per frame a torch.cat of the tiles' offset boxes and scores and one mdcv_nms (the counts GIVEN to the host for free, which that assembly
would first have to read back).

usage: tiles_probe.py [frames (default 32)] [rounds (default 3)]   |   tiles_probe.py merge [candidates per tile (default 40)]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import detect_rate as R  # noqa: E402
from mdcv import _lib  # noqa: E402
from mdcv.data import images as I  # noqa: E402
from mdcv.yolo.detect import FrameDetector, TiledBatchPlan, TiledFrameDetector  # noqa: E402


def rates(n, rounds):
    model, frames = R.make_model(), R.make_frames(n)
    geoms = [I.sample_geometry(R.FW, R.FH, 416, 416, ts=False) for _ in range(4)]
    with torch.no_grad():
        obj = model(I.transform_batch(frames[:4], geoms))[..., 4].float()
    top = torch.sort(obj, dim=1, descending=True)[0]
    conf = float(top[:, 40].min())
    if float(top[:, 0].min()) <= conf:
        below = obj[obj < conf]
        assert below.numel() > 0, "the objectness is one value everywhere: no threshold selects boxes"
        conf = float(below.max())
    nms_thres = model.get_threshs()[1]
    whole = FrameDetector(model, conf_thres=conf, nms_thres=nms_thres, batch_size=R.BATCH)
    tiled = TiledFrameDetector(model, 1.0, conf_thres=conf, nms_thres=nms_thres, batch_size=R.BATCH)
    seam = TiledFrameDetector(model, 1.0, conf_thres=conf, nms_thres=nms_thres, batch_size=R.BATCH, contain_thres=0.6)
    paths = {"w": lambda: [len(r.boxes) for r in whole.detect_frames(frames)],
             "t": lambda: [len(r.boxes) for r in tiled.detect_frames(frames)],
             "s": lambda: [len(r.boxes) for r in seam.detect_frames(frames)]}
    res = {k: fn() for k, fn in paths.items()}                                    # warm-up: plans, pinned buffers
    t = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            t[k].append(R.timed(fn)[0])
    tiles = TiledBatchPlan([(R.FW, R.FH)], 416, 416, 200, [1.0]).NT
    print(f"yolo_baseline 416x416 bf16, {n} frames of {R.FW}x{R.FH} ({tiles} tiles each at scale 1.0), conf_thres {conf:.4f}, nms_thres {nms_thres}, "
          f"{rounds} alternated rounds (frames/s per round; median)")
    what = {"w": "FrameDetector, whole frame        ", "t": "TiledFrameDetector, scale 1.0     ", "s": "the same, contain_thres 0.6       "}
    med = {}
    for k in paths:
        r = sorted(n / v for v in t[k])
        med[k] = r[len(r) // 2]
        print(f"    ({k}) {what[k]} " + " / ".join(f"{n / v:8.1f}" for v in t[k]) + f"   median {med[k]:8.1f} frames/s ({1e3 / med[k]:7.2f} ms per frame, "
              f"{1e3 / med[k] / (tiles if k != 'w' else 1):6.2f} ms per network input)   boxes kept {sum(res[k])}")
    print(f"    (w) / (t) = {med['w'] / med['t']:.2f}x for {tiles}x the network inputs")


def merge(per):
    L = _lib.lib()
    B, K, cols, rows = R.BATCH, 200, 5, 3
    T = B * cols * rows
    rng = np.random.default_rng(3)
    c, s = rng.uniform(0, 416, (T, K, 2)), rng.uniform(8, 60, (T, K, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2], axis=2).astype(np.float32)
    prob = -np.sort(-((rng.permutation(T * K) + 1.0) / (T * K + 1.0)).astype(np.float32).reshape(T, K), axis=1)       # distinct scores
    count = np.full(T, per, np.int32)
    tiles = np.array([[t // (cols * rows), 376 * (t % cols), 392 * ((t // cols) % rows), 0] for t in range(T)], np.int32)
    d_boxes, d_prob, d_count, d_tiles = (torch.from_numpy(a).cuda() for a in (boxes, prob, count, tiles))
    ob = torch.empty(B, K, 4, device="cuda")
    op = torch.empty(B, K, device="cuda")
    src = torch.empty(B, K, 2, dtype=torch.int32, device="cuda")
    cnt = torch.empty(B, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def one_launch():
        L.check(L.detect_merge_tiles(d_boxes.data_ptr(), d_prob.data_ptr(), d_count.data_ptr(), tiles.ctypes.data, d_tiles.data_ptr(), T, K, B, 0.5,
                                     -1.0, K, ob.data_ptr(), op.data_ptr(), src.data_ptr(), cnt.data_ptr(), st), "detect_merge_tiles")

    offs = torch.from_numpy(tiles[:, [1, 2, 1, 2]].astype(np.float32)).cuda()
    n = cols * rows * per
    keep = torch.empty(B, K, dtype=torch.long, device="cuda")
    kcnt = torch.empty(B, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(L.nms_workspace_bytes(n)), dtype=torch.uint8, device="cuda")

    def pieces():
        for b in range(B):
            t0 = b * cols * rows
            cand = torch.cat([d_boxes[t, :per] + offs[t] for t in range(t0, t0 + cols * rows)])
            score = torch.cat([d_prob[t, :per] for t in range(t0, t0 + cols * rows)])
            L.check(L.nms(cand.data_ptr(), score.data_ptr(), n, 0.5, K, keep[b].data_ptr(), kcnt[b:].data_ptr(), ws.data_ptr(), st), "nms")

    us = {}
    for name, fn, iters in (("merge", one_launch, 200), ("pieces", pieces, 20)):
        fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        e.synchronize()
        us[name] = 1e3 * s.elapsed_time(e) / iters
    assert np.array_equal(cnt.cpu().numpy(), kcnt.cpu().numpy()), "the two merges keep different numbers of boxes"
    print(f"mdcv_detect_merge_tiles B={B} x {cols * rows} tiles, K=top_k={K}, {per} candidates per tile ({n} per frame), kept per frame "
          f"{cnt.float().mean().item():.1f}: one launch {us['merge']:.2f} us; per-frame torch.cat + mdcv_nms ({B} x ({cols * rows + 2} torch "
          f"launches + 2 kernels), counts given) {us['pieces']:.2f} us; ratio {us['pieces'] / us['merge']:.1f}x (back-to-back, device events)")


if __name__ == "__main__":
    torch.cuda.set_device(0)
    if len(sys.argv) > 1 and sys.argv[1] == "merge":
        merge(int(sys.argv[2]) if len(sys.argv) > 2 else 40)
    else:
        rates(int(sys.argv[1]) if len(sys.argv) > 1 else 32, int(sys.argv[2]) if len(sys.argv) > 2 else 3)
