"""What Soft-NMS costs, on the benchmark's post-processing workload: bench.py's synthetic eval output [32, 10647, 85] with 16
label rows per image, NMS 0.25, IoU 0.5.

    softnms_cost.py [reps]
        `detect_postprocess` with nms="hard" (today's path), "linear" and "gaussian" on the same tensors, at top_k 200 and 512, at the
        benchmark's conf_thres 0.8 and at conf_thres 0.001 (every image fills top_k, so the soft scan runs its most rounds): device events
        around `reps` back-to-back calls, the three paths alternating for five windows each; then the kept counts, which for a soft
        method are the rounds of the scan."""
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
    for top_k in (200, 512):
        paths = {m: (lambda m=m: detect_postprocess(out, tg, conf, 0.25, 0.5, 416, 416, top_k, nms=m)) for m in ("hard", "linear", "gaussian")}
        for fn in paths.values():
            for _ in range(10):
                fn()
        res = {k: [] for k in paths}
        for _ in range(5):
            for name, fn in paths.items():
                res[name].append(window(fn))
        for name, fn in paths.items():
            t, det = res[name], fn()
            print("conf_thres %-5g top_k %3d %-8s median %7.1f us (%s)  kept %d of %d images, most %d, correct %d" % (
                conf, top_k, name, statistics.median(t), " ".join("%.1f" % v for v in t), int(det.count.sum()), B, int(det.count.max()),
                int(det.correct.sum())), flush=True)
