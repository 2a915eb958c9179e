"""What mosaic augmentation costs, on YOLOv3 416² B=32 (BASELINE config 3), one process.

    mosaic_cost.py kernel [reps]
        `mdcv_mosaic_batch` alone at B=32, 3x416², T=16 -> T_out=64: device events around `reps` back-to-back launches, five times, against
        the byte floor 2·B·C·H·W·4 (every pixel read once and written once) at the 8.0 TB/s spec rate and at the rate of a device copy
        measured here (bench.py's `peaks` probe), and beside a torch copy of the same batch.
    mosaic_cost.py step [rounds] [steps]
        the SyntheticCones-fed training step with and without the wrapper, two models, timed alternately for `rounds` rounds of `steps` steps."""
import os, statistics, sys, tempfile, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from mdcv import _lib
from mdcv.data import MosaicBatches, SyntheticCones
from mdcv.data.mosaic import draw_rows

mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
dev = torch.device("cuda", 0)
B, C, H, W, T = 32, 3, 416, 416, 16


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
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    A = _lib.aug_lib()
    _, x, tg = SyntheticCones(B, H, W, T, device=dev).batch(0)
    rows = np.asarray(draw_rows(0, 1, 0, B, H, W), np.int32)
    desc = torch.from_numpy(rows).to(dev)
    out, tout = torch.empty_like(x), torch.empty(B, 4 * T, 5, device=dev)
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def launch():
        A.check(A.mosaic_batch(rows.ctypes.data, desc.data_ptr(), B, C, H, W, x.data_ptr(), out.data_ptr(), tg.data_ptr(), T, tout.data_ptr(),
                               4 * T, 2.0, 0.25, stats.data_ptr(), s), "mosaic_batch")
    t_k = timed(launch, reps)
    t_c = timed(lambda: out.copy_(x), reps)
    hbm = bench.measured_peaks().get("measured_hbm_gbs")
    byt = 2 * B * C * H * W * 4
    med = statistics.median(t_k)
    print("mosaic_batch alone    median %.1f us (%s): %.2f TB/s read + written; byte floor %.1f MB at 8.0 TB/s %.1f us -> %.2fx"
          % (med, " ".join("%.1f" % v for v in t_k), byt / med / 1e6, byt / 1e6, byt / 8.0e6, med / (byt / 8.0e6))
          + ("" if not hbm else "; at the %.2f TB/s a 1 GiB copy reaches here %.1f us -> %.2fx" % (hbm / 1e3, byt / (hbm * 1e3), med / (byt / (hbm * 1e3)))))
    print("torch copy of the batch median %.1f us (%s): %.2f TB/s read + written" % (statistics.median(t_c), " ".join("%.1f" % v for v in t_c),
                                                                                      byt / statistics.median(t_c) / 1e6))
    print("counters after %d launches: %s" % (5 * reps + 5, stats.cpu().tolist()))
else:
    from mdcv.optim import FusedAdam
    from mdcv.yolo.models import Darknet
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 40
    tmp = tempfile.mkdtemp()

    def make(wrap):
        cfg = bench.write_yolo_cfg(tmp)
        os.chdir(tmp)
        torch.manual_seed(0)
        net = Darknet(cfg, 2.0, 1.6, 25.0, 0.1, True).to(dev).train()
        opt = FusedAdam(net, lr=1e-3)
        loader = SyntheticCones(B, H, W, T, batches=steps, device=dev)
        if wrap:
            loader = MosaicBatches(loader)

        def epoch(n):
            for i, (_, x, tg) in enumerate(loader):
                if i >= n:
                    break
                opt.zero_grad()
                net(x, tg)[0].sum().backward()
                opt.step()
        epoch(6)
        return loader, epoch

    cases = {"SyntheticCones": make(False), "MosaicBatches(SyntheticCones)": make(True)}
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
        print("%-32s median %.3f ms  min %.3f  (%s)  %.0f img/s" % (name, statistics.median(t), min(t), " ".join("%.3f" % v for v in t),
                                                                    B / statistics.median(t) * 1e3), flush=True)
    print("mosaic counters:", cases["MosaicBatches(SyntheticCones)"][0].stats(), flush=True)
