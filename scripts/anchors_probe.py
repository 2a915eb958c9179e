"""Times the anchor k-means (csrc/anchors.hip) at a size a dataset has: N = 200 000 boxes, K = 9 ("Dataset preparation").

    python scripts/anchors_probe.py [--n 200000] [--k 9] [--out profiles/anchors_probe.txt] [--reference <reference checkout>]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/anchors_probe.py --restarts 1 --steps 300 --steps-only     (kernel times alone)

  - us per iteration for R = 1 and R = 64: device events around `--steps` blind iterations enqueued in one mdcv_kmeans_steps call after a
    warm-up call, five windows each, median and range (no host read inside a window)
  - wall time of a full kmeans_anchors run (host clock around the call; it ends in the last chunk's synchronise), R = 1 and R = 64, with
    the iteration counts, and the same with check_every = 1
  - with --reference: one `assignment` + `update` of the reference's own functions on this host's CPU, same boxes

The boxes are seeded and have the form prepare_dataset produces, fl(fl(k * ratio) + min_cone)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def boxes(n, seed=0):
    rng = np.random.default_rng(seed)
    h = rng.integers(6, 420, n)
    w = np.maximum(3, (h * rng.uniform(0.45, 0.95, n)).astype(np.int64))
    ratio = 73 / 211
    return np.stack([(h - 14) * ratio + 10, (w - 9) * ratio + 10], 1)


def time_steps(L, torch, pts, K, R, steps, windows=5):
    from mdcv.data import prep
    n = len(pts)
    d_pts = torch.from_numpy(pts).cuda()
    d_init = torch.from_numpy(prep.initial_indices(n, K, 0, R)).cuda()
    ws = torch.empty(L.kmeans_workspace_bytes(n, K, R) // 8, dtype=torch.int64, device="cuda")
    asg = torch.empty(R * n, dtype=torch.uint8, device="cuda")
    rec = torch.empty(R * (prep.REC_HEAD + 2 * K), dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L.check(L.kmeans_begin(ws.data_ptr(), d_pts.data_ptr(), d_init.data_ptr(), n, K, R, st), "begin")
    L.check(L.kmeans_steps(ws.data_ptr(), d_pts.data_ptr(), asg.data_ptr(), rec.data_ptr(), n, K, R, 0, steps, st), "warm-up")
    torch.cuda.synchronize()
    done, out = steps, []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(L.kmeans_steps(ws.data_ptr(), d_pts.data_ptr(), asg.data_ptr(), rec.data_ptr(), n, K, R, done, steps, st), "steps")
        e1.record()
        e1.synchronize()
        done += steps
        out.append(e0.elapsed_time(e1) * 1e3 / steps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--k", type=int, default=9)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--restarts", default="1,64", help="the R values to time")
    ap.add_argument("--steps-only", action="store_true", help="skip the whole kmeans_anchors runs (kernel traces)")
    ap.add_argument("--reference", default=None)
    opt = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    pts = boxes(opt.n)
    say(f"anchors_probe: N = {opt.n}, K = {opt.k}, {opt.steps} steps per window")
    if opt.reference:
        import types
        import pandas as pd
        sys.modules.setdefault("cv2", types.ModuleType("cv2"))
        sys.path.insert(0, os.path.join(opt.reference, "CVC-YOLOv3"))
        import generate_kmeans_dataset_csvs as ref
        from mdcv.data import prep
        df = pd.DataFrame({"h": pts[:, 0], "w": pts[:, 1]})
        cent = {i: [pts[j, 0], pts[j, 1]] for i, j in enumerate(prep.initial_indices(opt.n, opt.k, 0, 1)[0])}
        df = ref.assignment(df, cent)
        ts = []
        for _ in range(3):
            t = time.perf_counter()
            cent = ref.update(df, cent)
            df = ref.assignment(df, cent)
            ts.append(time.perf_counter() - t)
        say(f"reference assignment + update on this host's CPU: {min(ts):.3f} s per iteration (best of 3)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("anchors_probe: no GPU; nothing is timed without one")
    from mdcv import _lib
    from mdcv.data import kmeans_anchors
    L = _lib.lib()
    restarts = [int(r) for r in opt.restarts.split(",")]
    for R in restarts:
        us = time_steps(L, torch, pts, opt.k, R, opt.steps)
        say(f"R = {R:2d}: {statistics.median(us):8.2f} us per iteration (median of {len(us)} windows, {min(us):.2f} .. {max(us):.2f}); "
            f"{statistics.median(us) / R:.2f} us per iteration and restart")
    for R in ([] if opt.steps_only else restarts):
        for every in (8, 1):
            kmeans_anchors(pts[:1000], opt.k, restarts=R)                       # warm-up of the path, not of this shape's result
            t = time.perf_counter()
            km = kmeans_anchors(pts, opt.k, restarts=R, check_every=every)
            dt = time.perf_counter() - t
            say(f"kmeans_anchors R = {R:2d}, check_every = {every}: {dt * 1e3:8.1f} ms wall; iterations of the restarts "
                f"{int(km.all_iterations.min())} .. {int(km.all_iterations.max())}, best restart {km.best} with {km.iterations}; "
                f"distortion best / restart 0 = {km.distortions[km.best] / km.distortions[0]:.6f}")
    if opt.out:
        with open(opt.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
