"""What key-point augmentation costs, on RektNet 80x80 B=256 (the benchmark's key-point configuration), one process.

    kptaug_cost.py kernel [reps]
        `mdcv_kptaug_batch` alone at B=256, 3x80², every image augmented (the wrapper's default draws on centred points, which no draw
        rejects), then every image passed through: device events around `reps` back-to-back launches, five windows each, against the byte
        floor -- read 3·S²·4, write (3 + 7)·S²·4 bytes per augmented image -- at the 5.2 TB/s copy rate the project prices with and at
        the rate of a device copy measured here (bench.py's `peaks` probe), and beside torch copies of the three tensors.
    kptaug_cost.py step [rounds] [steps]
        the SyntheticConeCrops-fed training step with and without the wrapper, two models, timed alternately for `rounds` rounds of
        `steps` steps; the run without the wrapper is the loop as it was before the wrapper existed."""
import contextlib, io, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from mdcv import _lib
from mdcv.data import KeypointAugBatches, SyntheticConeCrops
from mdcv.data.kptaug import draw_rows

mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
dev = torch.device("cuda", 0)
B, C, S = 256, 3, 80
COPY_TBS = 5.2


def timed(fn, reps):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(5):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    return out


if mode == "kernel":
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    A = _lib.kptaug_lib()
    x, hm, _, _, _ = SyntheticConeCrops(B, device=dev).batch(0)
    pts = torch.full((B, 7, 2), 0.5, device=dev)
    outs = [torch.empty_like(t) for t in (x, hm, pts)]
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    hbm = bench.measured_peaks().get("measured_hbm_gbs")
    floor_b = B * (C + C + 7) * S * S * 4
    for name, rows in (("every image augmented", draw_rows(0, 1, 0, B, S)), ("every image passed through", draw_rows(0, 1, 0, B, S, p=0.0))):
        desc = torch.from_numpy(rows).to(dev)
        stats.zero_()

        def launch():
            A.check(A.kptaug_batch(rows.ctypes.data, desc.data_ptr(), B, C, S, 7, x.data_ptr(), hm.data_ptr(), pts.data_ptr(),
                                   *[o.data_ptr() for o in outs], stats.data_ptr(), s), "kptaug_batch")
        t = timed(launch, reps)
        med = statistics.median(t)
        byt = floor_b if name.endswith("augmented") else 2 * B * (C + 7) * S * S * 4
        print("kptaug_batch, %-27s median %.1f us (%s): %.2f TB/s of its byte floor %.1f MB; the floor at %.1f TB/s is %.1f us -> %.2fx"
              % (name + ":", med, " ".join("%.1f" % v for v in t), byt / med / 1e6, byt / 1e6, COPY_TBS, byt / (COPY_TBS * 1e6), med / (byt / (COPY_TBS * 1e6)))
              + ("" if not hbm else "; at the %.2f TB/s a 1 GiB copy reaches here %.1f us -> %.2fx" % (hbm / 1e3, byt / (hbm * 1e3), med / (byt / (hbm * 1e3)))))
        print("   counters after %d launches: %s" % (5 * reps + 5, stats.cpu().tolist()))

    def copies():
        for o, t in zip(outs, (x, hm, pts)):
            o.copy_(t)
    t_c = timed(copies, reps)
    byt = 2 * B * (C + 7) * S * S * 4
    print("torch copies of the three tensors median %.1f us (%s): %.2f TB/s read + written" % (statistics.median(t_c), " ".join("%.1f" % v for v in t_c),
                                                                                                byt / statistics.median(t_c) / 1e6))
else:
    from mdcv.optim import FusedAdam
    from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss
    from mdcv.rektnet.keypoint_net import KeypointNet
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 100

    def make(wrap):
        torch.manual_seed(0)
        net = KeypointNet(7, (80, 80), precision="bf16").to(dev).train()
        with contextlib.redirect_stdout(io.StringIO()):
            crit = CrossRatioLoss("l1_softargmax", True, 0.05, 0.05)
        opt = FusedAdam(net, lr=1e-3)
        loader = SyntheticConeCrops(B, batches=steps, device=dev)
        if wrap:
            loader = KeypointAugBatches(loader)

        def epoch(n):
            for i, (x, hm, pts, _, _) in enumerate(loader):
                if i >= n:
                    break
                opt.zero_grad()
                out = net(x)
                crit(out[0], out[1], hm, pts)[2].backward()
                opt.step()
        epoch(6)
        return loader, epoch

    cases = {"SyntheticConeCrops": make(False), "KeypointAugBatches(SyntheticConeCrops)": make(True)}
    torch.cuda.synchronize()
    res = {k: [] for k in cases}
    for rnd in range(rounds):
        for name, (loader, epoch) in cases.items():
            epoch(3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            epoch(steps)
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / steps * 1e3)
    for name, t in res.items():
        print("%-40s median %.3f ms  min %.3f  (%s)  %.0f img/s" % (name, statistics.median(t), min(t), " ".join("%.3f" % v for v in t),
                                                                    B / statistics.median(t) * 1e3), flush=True)
    print("augmentation counters:", cases["KeypointAugBatches(SyntheticConeCrops)"][0].stats(), flush=True)
