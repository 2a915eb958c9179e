"""What the dataset-level evaluator costs: one `DatasetAP.add` at B = 32, K = 200, T = 64, J = 10, S = 4 next to the
`detect_postprocess` call it follows, on the same batch, and `result()` over 10 000 images.  Event timings after a warm-up, the median of
the repeats.  python scripts/detmap_probe.py [--repeats 50]"""
import argparse
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdcv.yolo import DatasetAP  # noqa: E402
from mdcv.yolo.postprocess import detect_postprocess  # noqa: E402

RANGES = ((0.0, math.inf), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, math.inf))


def median_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=50)
    p.add_argument("--images", type=int, default=10000)
    a = p.parse_args()
    B, K, T, N, side = 32, 200, 64, 2000, 416.0
    g = torch.Generator(device="cuda").manual_seed(0)
    pred = torch.rand(B, N, 6, device="cuda", generator=g)
    pred[..., 0:2] *= side
    pred[..., 2:4] = 10 + 50 * pred[..., 2:4]
    targets = torch.zeros(B, T, 5, device="cuda")
    targets[:, :30, 1:3] = 0.1 + 0.8 * torch.rand(B, 30, 2, device="cuda", generator=g)
    targets[:, :30, 3:5] = 0.03 + 0.1 * torch.rand(B, 30, 2, device="cuda", generator=g)
    post = lambda: detect_postprocess(pred, targets, 0.5, 0.45, 0.5, side, side, K)      # noqa: E731
    det = post()
    cap = (a.images + B - 1) // B * B
    acc = DatasetAP(1, cap, top_k=K, area_ranges=RANGES)

    def add():
        acc.n_images = 0
        acc.add(det, targets, side, side)
    print(f"batch: B {B}, K {K}, T {T}, J {acc.J}, S {acc.S}; kept per image {det.count.float().mean().item():.1f}")
    m, lo, hi = median_ms(post, 5, a.repeats)
    print(f"detect_postprocess   median {1e3 * m:8.1f} us  (min {1e3 * lo:.1f}, max {1e3 * hi:.1f})")
    m, lo, hi = median_ms(add, 5, a.repeats)
    print(f"DatasetAP.add        median {1e3 * m:8.1f} us  (min {1e3 * lo:.1f}, max {1e3 * hi:.1f})")
    acc.reset()
    for _ in range(cap // B):
        acc.add(det, targets, side, side)
    torch.cuda.synchronize()
    m, lo, hi = median_ms(acc.result, 2, max(a.repeats // 10, 5))
    t0 = time.perf_counter()
    r = acc.result()
    wall = time.perf_counter() - t0
    print(f"result() over {acc.n_images} images   median {m:8.2f} ms  (min {lo:.2f}, max {hi:.2f}); wall clock of one call {1e3 * wall:.2f} ms")
    print(r.summary())


if __name__ == "__main__":
    main()
