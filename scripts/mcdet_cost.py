"""What the class-aware detection post-processing costs, on the benchmark's post-processing workload: bench.py's synthetic
eval output [32, 10647, 85] with 16 label rows per image, NMS 0.25, IoU 0.5, top_k 200.

    mcdet_cost.py [reps]
        `detect_postprocess(class_aware=True)` beside the class-agnostic call on the same tensors, at the benchmark's conf_thres 0.8 and
        at conf_thres 0.001 (every row's class words are read): device events around `reps` back-to-back calls, the two paths
        alternating for five windows each; then the kept counts of both, so that the two loads can be compared."""
import os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from mdcv.yolo.postprocess import detect_postprocess

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
dev = torch.device("cuda", 0)
B, N, C, T = 32, 10647, 80, 16
out_np, tg_np = bench.synth_eval_output(B, N, C, T, 3000)
out, tg = torch.from_numpy(out_np).to(dev), torch.from_numpy(tg_np).to(dev)


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


for conf in (0.8, 0.001):
    paths = {"class-agnostic": lambda: detect_postprocess(out, tg, conf, 0.25, 0.5, 416, 416),
             "class_aware=True": lambda: detect_postprocess(out, tg, conf, 0.25, 0.5, 416, 416, class_aware=True)}
    for fn in paths.values():
        for _ in range(10):
            fn()
    res = {k: [] for k in paths}
    for _ in range(5):
        for name, fn in paths.items():
            res[name].append(window(fn))
    for name, fn in paths.items():
        t, det = res[name], fn()
        print("conf_thres %-5g %-17s median %7.1f us (%s)  kept %d, correct %d" % (
            conf, name, statistics.median(t), " ".join("%.1f" % v for v in t), int(det.count.sum()), int(det.correct.sum())), flush=True)
