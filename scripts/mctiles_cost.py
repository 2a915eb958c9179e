"""What the class-aware tile merge costs.

    mctiles_cost.py [reps]
        1. the merge launch alone: B = 16 frames of 16 tiles (a 4 x 4 grid of 416 x 416 tiles that overlap by 66 px), K = top_k = 200,
           every slot a candidate (3200 per frame, cut to 200), contain_thres off and 0.6, the classes all equal and drawn from eight.  mdcv_detect_merge_tiles_mc beside the class-agnostic mdcv_detect_merge_tiles on the same device tensors (its
           code is the parent commit's): device events around `reps` back-to-back calls, the two alternating for five windows each;
           median and all windows, then the kept counts of both.
        2. end to end: `TiledFrameDetector.detect_frames` over 16 frames (the four golden frames, four times: 168 tiles of 64 x 64) on the
           mini model, tile_merge="per_class" beside the default, a host clock around whole calls (they end in the batch's
           synchronisation), alternating for five windows each."""
import os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdcv import _lib
from mdcv.yolo.detect import TiledFrameDetector
from mdcv.yolo.models import Darknet

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
dev = torch.device("cuda", 0)
B, TPF, K = 16, 16, 200
T = B * TPF


def inputs(ncls, seed=35):
    """boxes of 20..80 px anywhere in a 416 x 416 tile, the tiles of a frame 350 px apart (66 px of overlap), scores descending per tile"""
    rng = np.random.default_rng(seed)
    c, s = rng.uniform(0, 416, (T, K, 2)), rng.uniform(20, 80, (T, K, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2], axis=2).astype(np.float32)
    prob = -np.sort(-rng.uniform(0.05, 0.95, (T, K)).astype(np.float32), axis=1)
    cls = rng.integers(0, ncls, (T, K)).astype(np.int32)
    tiles = np.array([[t // TPF, 350 * (t % 4), 350 * (t % TPF // 4), 0] for t in range(T)], np.int32)
    return boxes, prob, cls, np.full(T, K, np.int32), tiles


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def report(what, paths, measure):
    for fn in paths.values():
        measure(fn, 10)
    res = {k: [] for k in paths}
    for _ in range(5):
        for name, fn in paths.items():
            res[name].append(measure(fn, reps))
    for name, t in res.items():
        print("%-34s %-12s median %8.1f us (%s)  %s" % (what, name, statistics.median(t), " ".join("%.1f" % v for v in t), paths[name]()), flush=True)


st = torch.cuda.current_stream(dev).cuda_stream
for ncls in (1, 8):
    boxes, prob, cls, count, tiles = inputs(ncls)
    d = [torch.from_numpy(a.reshape(-1)).to(dev) for a in (boxes, prob, cls, count, tiles)]
    ob, op, oc = torch.empty(B, K, 4, device=dev), torch.empty(B, K, device=dev), torch.empty(B, K, dtype=torch.int32, device=dev)
    osrc, ocnt = torch.empty(B, K, 2, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    for contain in (-1.0, 0.6):
        def agnostic():
            L = _lib.lib()
            L.check(L.detect_merge_tiles(d[0].data_ptr(), d[1].data_ptr(), d[3].data_ptr(), tiles.ctypes.data, d[4].data_ptr(), T, K, B, 0.5,
                                         contain, K, ob.data_ptr(), op.data_ptr(), osrc.data_ptr(), ocnt.data_ptr(), st), "detect_merge_tiles")
            return ""

        def per_class():
            L = _lib.mctiles_lib()
            L.check(L.detect_merge_tiles_mc(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), tiles.ctypes.data, d[4].data_ptr(),
                                            T, K, B, 0.5, contain, K, ob.data_ptr(), op.data_ptr(), oc.data_ptr(), osrc.data_ptr(),
                                            ocnt.data_ptr(), st), "detect_merge_tiles_mc")
            return ""
        report("merge alone, %d class%s, contain %-4g" % (ncls, "" if ncls == 1 else "es", contain), {"agnostic": agnostic, "per_class": per_class}, window)
        kept = {}
        for name, fn in (("agnostic", agnostic), ("per_class", per_class)):
            fn()
            kept[name] = int(ocnt.sum())
        print("    kept boxes over the %d frames: %s" % (B, kept), flush=True)

# ---- end to end on the mini model
cwd = os.getcwd()
os.chdir(os.path.join(ROOT, "tests", "golden", "mini"))
net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32")
net.load_weights("mini.weights", net.get_start_weight_dim())
os.chdir(cwd)
net = net.to(dev).eval()
z = np.load(os.path.join(ROOT, "tests", "golden", "imgload", "frames.npz"))
frames = [np.ascontiguousarray(z[k]) for k in sorted(z.files)] * 4
dets = {"default": TiledFrameDetector(net, 1.0, conf_thres=0.05, contain_thres=0.6),
        "per_class": TiledFrameDetector(net, 1.0, conf_thres=0.05, contain_thres=0.6, class_aware=True, tile_merge="per_class")}
reps = max(reps // 50, 5)


def clock(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n * 1e6


report("detect_frames, 16 frames, mini", {k: (lambda det=det: "boxes %d" % sum(len(r.boxes) for r in det.detect_frames(frames))) for k, det in dets.items()}, clock)
