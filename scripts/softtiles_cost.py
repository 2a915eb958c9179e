"""What the soft cross-tile merge costs, on §35's shape: B = 16 frames of 16 tiles (a 4 x 4 grid of 416 x 416 tiles that
overlap by 66 px), K = 200, every slot a candidate (3200 per frame), classes drawn from eight, contain_thres 0.6.

    softtiles_cost.py [reps]
        1. the merge launch alone at top_k 200 and 512: mdcv_detect_merge_tiles and mdcv_detect_merge_tiles_mc as they stand, and
           mdcv_detect_merge_tiles_soft with hard, linear and Gaussian, both class flags, at score_thres 0.9 (the scan stops early) and -1
           (every round runs): device events around `reps` back-to-back calls, the paths alternating for five windows each; median, all
           windows; the rounds (the emitted counts) of the longest and of all frames are read once, behind the windows.  Time per round =
           all-rounds time / longest scan.
        2. end to end: `TiledFrameDetector.detect_frames` over 16 frames (the four golden frames, four times) on the mini model,
           nms="linear" with tile_merge="soft" beside the defaults, a host clock around whole calls, alternating for five windows each."""
import os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from mdcv import _lib
from mdcv.yolo.detect import TiledFrameDetector
from mdcv.yolo.models import Darknet

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
dev = torch.device("cuda", 0)
B, TPF, K = 16, 16, 200
T = B * TPF
rng = np.random.default_rng(35)
c, s = rng.uniform(0, 416, (T, K, 2)), rng.uniform(20, 80, (T, K, 2))
boxes = np.concatenate([c - s / 2, c + s / 2], axis=2).astype(np.float32)
prob = -np.sort(-rng.uniform(0.05, 0.95, (T, K)).astype(np.float32), axis=1)
cls = rng.integers(0, 8, (T, K)).astype(np.int32)
tiles = np.array([[t // TPF, 350 * (t % 4), 350 * (t % TPF // 4), 0] for t in range(T)], np.int32)
d = [torch.from_numpy(a.reshape(-1)).to(dev) for a in (boxes, prob, cls, np.full(T, K, np.int32), tiles)]
st = torch.cuda.current_stream(dev).cuda_stream


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def report(what, paths, measure, n, after):
    for fn in paths.values():
        measure(fn, 5)
    res = {k: [] for k in paths}
    for _ in range(5):
        for name, fn in paths.items():
            res[name].append(measure(fn, n))
    for name, t in res.items():
        paths[name]()
        print("%-22s %-26s median %8.1f us (%s)  %s" % (what, name, statistics.median(t), " ".join("%.1f" % v for v in t), after()), flush=True)


for top_k in (200, 512):
    ob, op = torch.empty(B, top_k, 4, device=dev), torch.empty(B, top_k, device=dev)
    oc, osrc = torch.empty(B, top_k, dtype=torch.int32, device=dev), torch.empty(B, top_k, 2, dtype=torch.int32, device=dev)
    ocnt = torch.empty(B, dtype=torch.int32, device=dev)
    rounds = lambda: "rounds: longest %d, all %d" % (int(ocnt.max()), int(ocnt.sum()))  # noqa: E731

    def agnostic():
        L = _lib.lib()
        L.check(L.detect_merge_tiles(d[0].data_ptr(), d[1].data_ptr(), d[3].data_ptr(), tiles.ctypes.data, d[4].data_ptr(), T, K, B, 0.5, 0.6,
                                     top_k, ob.data_ptr(), op.data_ptr(), osrc.data_ptr(), ocnt.data_ptr(), st), "detect_merge_tiles")

    def per_class():
        L = _lib.mctiles_lib()
        L.check(L.detect_merge_tiles_mc(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), tiles.ctypes.data, d[4].data_ptr(),
                                        T, K, B, 0.5, 0.6, top_k, ob.data_ptr(), op.data_ptr(), oc.data_ptr(), osrc.data_ptr(), ocnt.data_ptr(),
                                        st), "detect_merge_tiles_mc")

    def soft(method, aware, sthres):
        def call():
            L = _lib.softtiles_lib()
            L.check(L.detect_merge_tiles_soft(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr() if aware else None, d[3].data_ptr(),
                                              tiles.ctypes.data, d[4].data_ptr(), T, K, B, 0.5, 0.6, top_k, ob.data_ptr(), op.data_ptr(),
                                              oc.data_ptr() if aware else None, osrc.data_ptr(), ocnt.data_ptr(), method, 0.5, sthres, aware,
                                              st), "detect_merge_tiles_soft")
        return call
    paths = {"merge_tiles": agnostic, "merge_tiles_mc": per_class}
    for aware in (0, 1):
        paths["soft hard cls%d" % aware] = soft(0, aware, 0.0)
        for m, name in ((1, "linear"), (2, "gaussian")):
            for sthres in (0.9, -1.0):
                paths["soft %s cls%d thr %g" % (name, aware, sthres)] = soft(m, aware, sthres)
    report("merge alone, top_k %d" % top_k, paths, window, reps, rounds)

cwd = os.getcwd()
os.chdir(os.path.join(ROOT, "tests", "golden", "mini"))
net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32")
net.load_weights("mini.weights", net.get_start_weight_dim())
os.chdir(cwd)
net = net.to(dev).eval()
z = np.load(os.path.join(ROOT, "tests", "golden", "imgload", "frames.npz"))
frames = [np.ascontiguousarray(z[k]) for k in sorted(z.files)] * 4
dets = {"agnostic, nms hard": TiledFrameDetector(net, 1.0, conf_thres=0.05, contain_thres=0.6),
        "soft, nms linear": TiledFrameDetector(net, 1.0, conf_thres=0.05, contain_thres=0.6, nms="linear", tile_merge="soft")}


def clock(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n * 1e6


boxes = []
report("detect_frames, 16, mini", {k: (lambda det=det: boxes.append(sum(len(r.boxes) for r in det.detect_frames(frames)))) for k, det in dets.items()},
       clock, max(reps // 20, 5), lambda: "boxes %d" % boxes[-1])
