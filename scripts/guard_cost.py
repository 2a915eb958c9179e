"""What a gradient guard costs: the YOLOv3 416² B=32 training step (BASELINE config 3) with `guard=None` and with a
`GradGuard`, two models in one process, timed alternately; then the sum-of-squares launch and the finalize launch alone over that model's
flat gradient buffer, against the time the buffer's bytes need at the HBM rate.
usage: guard_cost.py [rounds] [steps] [pipeline 0|1]"""
import os, statistics, sys, tempfile, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from mdcv import _lib
from mdcv.optim import FusedAdam, GradGuard
from mdcv.yolo.models import Darknet

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
pipeline = bool(int(sys.argv[3])) if len(sys.argv) > 3 else False
dev = torch.device("cuda", 0)
tmp = tempfile.mkdtemp()
g = torch.Generator().manual_seed(1000)
x, tg = torch.rand(32, 3, 416, 416, generator=g).to(dev), bench.synth_targets(32, 16, g).to(dev)


def make(guard):
    cfg = bench.write_yolo_cfg(tmp)
    os.chdir(tmp)
    torch.manual_seed(0)
    net = Darknet(cfg, 2.0, 1.6, 25.0, 0.1, True).to(dev).train()
    opt = FusedAdam(net, lr=1e-3, pipeline=pipeline, guard=guard)

    def step():
        opt.zero_grad()
        loss = net(x, tg)[0].sum()
        loss.backward()
        opt.step()
        return loss
    for _ in range(6):
        step()
    return net, opt, step


cases = {"guard=None": make(None), "GradGuard(max_norm=10, skip_nonfinite=True)": make(GradGuard(max_norm=10.0, skip_nonfinite=True))}
torch.cuda.synchronize()
res = {k: [] for k in cases}
for rnd in range(rounds):
    for name, (net, opt, step) in cases.items():
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        res[name].append((time.perf_counter() - t0) / steps * 1e3)
for name, t in res.items():
    print("%-46s median %.3f ms  min %.3f  (%s)  %.0f img/s" % (name, statistics.median(t), min(t), " ".join("%.3f" % v for v in t),
                                                                32 / statistics.median(t) * 1e3), flush=True)
net, opt, _ = cases["GradGuard(max_norm=10, skip_nonfinite=True)"]
print("guard counters:", {k: v for k, v in opt.guard.stats().items() if k != "norms"}, flush=True)

# the two launches alone, device events around `reps` back-to-back launches
L = _lib.lib()
gflat = net.flat_parameters()[1]
n = gflat.numel()
guard = GradGuard()
guard.measure(gflat)
s = torch.cuda.current_stream().cuda_stream
nparts = (n + 4095) // 4096


def timed(fn, reps=50):
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


t_sum = timed(lambda: L.grad_sumsq(gflat.data_ptr(), n, guard._partials.data_ptr(), s))
t_fin = timed(lambda: L.grad_guard_finalize(guard._partials.data_ptr(), nparts, 1.0, 10.0, 1, 0.9, 0.999, guard.block_ptr, None, 0, s))
other = torch.empty_like(gflat)
t_copy = timed(lambda: other.copy_(gflat))
byt = n * 4
print("flat gradient: %d elements, %.1f MB, %d partials" % (n, byt / 1e6, nparts))
print("grad_sumsq alone      median %.1f us (%s): %.2f TB/s; byte floor at 8.0 TB/s %.1f us -> %.2fx; at the 6.29 TB/s this chip's copies reach %.1f us -> %.2fx"
      % (statistics.median(t_sum), " ".join("%.1f" % v for v in t_sum), byt / statistics.median(t_sum) / 1e6, byt / 8.0e6,
         statistics.median(t_sum) / (byt / 8.0e6), byt / 6.29e6, statistics.median(t_sum) / (byt / 6.29e6)))
print("finalize alone        median %.1f us (%s)" % (statistics.median(t_fin), " ".join("%.1f" % v for v in t_fin)))
print("device copy of it     median %.1f us: %.2f TB/s read + written" % (statistics.median(t_copy), 2 * byt / statistics.median(t_copy) / 1e6))
