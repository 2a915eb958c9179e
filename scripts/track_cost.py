"""What the tracker costs.

    track_cost.py [reps]
        1. mdcv_track_frames alone: one sequence of 32 frames from a fresh state (a 41 KB device copy resets it inside the timed window) at
           about 20, 100 and 256 boxes a frame (`synthetic_scene`: crossing boxes, 10 % misses, false positives), and 64 such sequences in
           one launch at 100: device events around `reps` back-to-back launches, five windows each after a warm-up; median and all
           windows, per frame; the longest augmenting path and the most scan steps of one frame's assignment are read once behind the
           windows.
        2. end to end: `FrameDetector.detect_frames` over 16 frames (the four golden frames, four times) on the mini model with and without
           `track` (without it the batch layout and every launch are the parent's), a host clock around whole calls that end in the
           detector's own synchronisation, alternating, five windows each."""
import os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdcv.yolo.detect import FrameDetector
from mdcv.yolo.models import Darknet
from mdcv.yolo.track import TrackConfig, TrackState, synthetic_scene, track_boxes

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
dev = torch.device("cuda", 0)
F = 32


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def clock(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n * 1e6


def report(what, paths, measure, n, after, per=1):
    for fn in paths.values():
        measure(fn, 5)
    res = {k: [] for k in paths}
    for _ in range(5):
        for name, fn in paths.items():
            res[name].append(measure(fn, n) / per)
    for name, t in res.items():
        paths[name]()
        print("%-30s %-16s median %9.2f us (%s)  %s" % (what, name, statistics.median(t), " ".join("%.2f" % v for v in t), after()), flush=True)


for objects, S in ((18, 1), (95, 1), (250, 1), (95, 64)):
    b, c, _ = synthetic_scene(F, objects, 39, size=(40 * objects ** 0.5 * 1.6, 40 * objects ** 0.5), false_pos=max(objects // 16, 1), K=256)
    boxes, count = torch.from_numpy(b).to(dev)[None].repeat(S, 1, 1, 1), torch.from_numpy(c).to(dev)[None].repeat(S, 1)
    state, cfg = TrackState(S, dev), TrackConfig()
    fresh = torch.zeros_like(state.raw)

    def run():
        state.raw.copy_(fresh)
        track_boxes(boxes, count, None, cfg, state)
    report("track_frames, S %d, boxes %.0f" % (S, c.mean()), {"per frame": run}, window, reps,
           lambda: "longest path %d, most scan steps in a frame %d, tracks opened %d" % (int(state.longest_path[0]), int(state.most_steps[0]), int(state.next_id[0])), per=F)

cwd = os.getcwd()
os.chdir(os.path.join(ROOT, "tests", "golden", "mini"))
net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32")
net.load_weights("mini.weights", net.get_start_weight_dim())
os.chdir(cwd)
net = net.to(dev).eval()
z = np.load(os.path.join(ROOT, "tests", "golden", "imgload", "frames.npz"))
frames = [np.ascontiguousarray(z[k]) for k in sorted(z.files)] * 4
dets = {"track=None": FrameDetector(net, conf_thres=0.05), "track=True": FrameDetector(net, conf_thres=0.05, track=True)}
seen = []
report("detect_frames, 16, mini", {k: (lambda det=det: seen.append(sum(len(r.boxes) for r in det.detect_frames(frames)))) for k, det in dets.items()},
       clock, max(reps // 10, 5), lambda: "boxes %d" % seen[-1])
