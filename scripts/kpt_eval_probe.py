"""Rates of RektNet validation on one GPU: the reference's batch-1 loop against mdcv.rektnet.eval_model (csrc/kpt_eval.hip), DESIGN 18.

1024 SyntheticConeCrops samples at 80x80, bf16, every path warmed up, the three paths alternated in one run; each timing is a host clock
around work that ends in a synchronise (or in the read-back eval_model ends with).

(a) the statements of the reference's eval_model (RektNet/train_eval.py:117-135) on the current classes, fed batches of 1: one B=1 plan,
    one CrossRatioLoss launch and three .item() per image -- what validation cost before mdcv.rektnet.evaluate existed
(b) mdcv.rektnet.eval_model fed the same batches of 1
(c) mdcv.rektnet.eval_model fed batches of 256

`kernel`: mdcv_kpt_eval_rows alone at B=256, l2_heatmap, 241 launches over rotated input sets -- for a `rocprofv3 --kernel-trace --stats`
run of its own; prints the byte floor (2 x 256 x 7 x 6400 x 4 B over the copy rate given in TB/s) and a device-event figure beside it.

usage: kpt_eval_probe.py [rounds (default 3)]   |   kpt_eval_probe.py kernel [TB/s (default 5.2)] [input sets (default 6)]"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdcv import _lib  # noqa: E402
from mdcv.data.synth import SyntheticConeCrops  # noqa: E402
from mdcv.rektnet import eval_model  # noqa: E402
from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss  # noqa: E402
from mdcv.rektnet.keypoint_net import KeypointNet  # noqa: E402

N, B, S = 1024, 256, 80


def reference_loop(model, batches, loss_function):
    model.eval()
    with torch.no_grad():
        loss_sums = [0, 0, 0]
        batch_num = 0
        for x_batch, y_hm_batch, y_point_batch, image_name, _ in batches:
            output = model(x_batch)
            loc_loss, geo_loss, loss = loss_function(output[0], output[1], y_hm_batch, y_point_batch)
            loss_sums[0] += loc_loss.item()
            loss_sums[1] += geo_loss.item()
            loss_sums[2] += loss.item()
            batch_num += 1
    return loss_sums[0] / batch_num, loss_sums[1] / batch_num, loss_sums[2] / batch_num


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def rates(rounds):
    big = list(SyntheticConeCrops(B, S, batches=N // B, seed=11))
    torch.cuda.synchronize()
    ones = [(x[i:i + 1], hm[i:i + 1], pts[i:i + 1], names[i:i + 1], sizes[i:i + 1]) for x, hm, pts, names, sizes in big for i in range(B)]
    torch.manual_seed(0)
    model = KeypointNet(7, (S, S), precision="bf16").cuda()
    devnull = open(os.devnull, "w")
    for lt in ("l1_softargmax", "l2_heatmap"):
        loss = CrossRatioLoss(lt, True, 0.05, 0.05)
        paths = {"a": lambda: reference_loop(model, ones, loss), "b": lambda: eval_model(model, ones, loss, (S, S)),
                 "c": lambda: eval_model(model, big, loss, (S, S))}
        stdout = sys.stdout
        sys.stdout = devnull                                   # eval_model's two lines, 2 x rounds times
        try:
            res = {k: fn() for k, fn in paths.items()}         # warm-up: plans, staging buffers
            t = {k: [] for k in paths}
            for _ in range(rounds):
                for k, fn in paths.items():
                    t[k].append(timed(fn)[0])
        finally:
            sys.stdout = stdout
        print(f"{lt}, {N} samples, bf16, {rounds} alternated rounds (img/s per round; median)")
        what = {"a": "reference loop at batch 1       ", "b": "eval_model, batches of 1       ", "c": f"eval_model, batches of {B}     "}
        med = {}
        for k in paths:
            r = sorted(N / v for v in t[k])
            med[k] = r[len(r) // 2]
            print(f"    ({k}) {what[k]} " + " / ".join(f"{N / v:9.0f}" for v in t[k]) + f"   median {med[k]:9.0f} img/s"
                  f" ({1e3 * N / med[k]:8.2f} ms per pass)   val loc/geo/total {res[k][0]:.6f} {res[k][1]:.6f} {res[k][2]:.6f}")
        print(f"    (c) / (a) = {med['c'] / med['a']:.1f}x   (b) / (a) = {med['b'] / med['a']:.1f}x")


def kernel(tbs, sets=6):
    """`sets` input sets of 91.8 MB each, walked round-robin.  Six sets: 550 MB between two reads of a byte, above the 256 MB Infinity
    Cache, so the figure is an HBM figure; one set re-reads what the cache may still hold"""
    g = torch.Generator().manual_seed(0)
    hm = [torch.softmax(torch.randn(B, 7, S * S, generator=g), -1).view(B, 7, S, S).cuda() for _ in range(sets)]
    thm = [torch.softmax(torch.randn(B, 7, S * S, generator=g) * 3, -1).view(B, 7, S, S).cuda() for _ in range(sets)]
    pts, tpts = torch.rand(B, 7, 2, generator=g).cuda(), torch.rand(B, 7, 2, generator=g).cuda()
    rows = torch.empty(B, 12, device="cuda")
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream

    def run(k):
        L.check(L.kpt_eval_rows(hm[k].data_ptr(), pts.data_ptr(), thm[k].data_ptr(), tpts.data_ptr(), B, S, S, 1, 1, 0.05, 0.05, 240.0, 240.0,
                                rows.data_ptr(), st), "kpt_eval_rows")

    def events(pick, iters=240):
        run(0)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for i in range(iters):
            run(pick(i))
        e.record()
        e.synchronize()
        return 1e3 * s.elapsed_time(e) / iters
    us = events(lambda i: i % sets)
    mb = 2 * B * 7 * S * S * 4 / 1e6
    floor = mb / tbs
    print(f"mdcv_kpt_eval_rows B={B} l2_heatmap {S}x{S}: {mb:.1f} MB read, byte floor {floor:.1f} us at {tbs} TB/s; back-to-back launches "
          f"(events) over {sets} rotated input set(s): {us:.1f} us = {us / floor:.2f} x floor")


if __name__ == "__main__":
    torch.cuda.set_device(0)
    if len(sys.argv) > 1 and sys.argv[1] == "kernel":
        kernel(float(sys.argv[2]) if len(sys.argv) > 2 else 5.2, int(sys.argv[3]) if len(sys.argv) > 3 else 6)
    else:
        rates(int(sys.argv[1]) if len(sys.argv) > 1 else 3)
