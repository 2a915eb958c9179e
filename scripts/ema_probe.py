"""What the weight EMA costs, on YOLOv3 416² B=32 bf16 (BASELINE config 3), one lease.

    ema_probe.py kernel [rounds] [reps]
        the flat update launch alone beside `adam_step` alone on the same flat buffer, alternately, device events around `reps` back-to-back
        launches.  The EMA moves 12 bytes per element (p and e read, e written), Adam 28: the yardstick is Adam's time x 12 / 28.
    ema_probe.py step [rounds] [steps] [--no-ema]
        the training step with `ema=None` and with a `WeightEMA`, `pipeline=False` and `pipeline=True`: one model per case in one process,
        timed alternately; then, on the full model, whether the pipelined shadow (late groups on the parameter stream) equals the plain one.
        `--no-ema`: only the two `ema=None` cases, through nothing this script's tree may lack -- the form to run from another checkout.
    ema_probe.py ab OTHER_TREE [rounds] [steps]
        `step --no-ema` from OTHER_TREE (a built checkout of the commit to compare with) and `step` from this tree, as fresh processes, alternately,
        twice each: EMA-off here against the other commit's step in one lease.

Every line of results is printed; nothing is asserted."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.environ.get("MDCV_PROBE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
flags = [a for a in sys.argv[1:] if a.startswith("--")]
mode = args[0] if args else "step"


def num(i, default):
    return int(args[i]) if len(args) > i else default


if mode == "ab":
    other = os.path.abspath(args[1])
    me = os.path.abspath(__file__)
    for rnd in range(2):
        for label, root, extra in (("other", other, ["--no-ema"]), ("this", ROOT, [])):
            print(f"---- round {rnd}: {label} tree ({root})", flush=True)
            env = dict(os.environ, MDCV_PROBE_ROOT=root)
            rc = subprocess.call([sys.executable, me, "step", str(num(2, 4)), str(num(3, 40))] + extra, env=env, cwd=root, timeout=600)
            if rc != 0:
                print(f"{label} tree: exit status {rc}; stopping", flush=True)
                sys.exit(rc)
    sys.exit(0)

sys.path.insert(0, ROOT)
import torch                                                            # noqa: E402
import bench                                                            # noqa: E402
from mdcv import _lib                                                   # noqa: E402
from mdcv.optim import FusedAdam                                        # noqa: E402
from mdcv.yolo.models import Darknet                                    # noqa: E402

dev = torch.device("cuda", 0)
tmp = tempfile.mkdtemp()
g = torch.Generator().manual_seed(1000)
x, tg = torch.rand(32, 3, 416, 416, generator=g).to(dev), bench.synth_targets(32, 16, g).to(dev)


def new_net():
    cfg = bench.write_yolo_cfg(tmp)
    os.chdir(tmp)
    torch.manual_seed(0)
    return Darknet(cfg, 2.0, 1.6, 25.0, 0.1, True).to(dev).train()


def timed(fn, reps, rounds=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(rounds):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    return out


if mode == "kernel":
    rounds, reps = num(1, 7), num(2, 50)
    L = _lib.lib()
    net = new_net()
    p, gr = net.flat_parameters()
    gr.normal_()
    n = p.numel()
    m, v, e = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    blk = torch.zeros(3, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    L.check(L.ema_advance(blk.data_ptr(), None, 0.9999, 10, s))
    cases = {
        "ema_update": lambda: L.ema_update(e.data_ptr(), p.data_ptr(), n, blk.data_ptr(), s),
        "adam_step": lambda: L.adam_step(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1, 1e-6, 0.9, 0.999, 1e-8, 0.0, 1.0, s),
        "ema_swap": lambda: L.ema_swap(e.data_ptr(), p.data_ptr(), n, s),
        "copy (p -> e)": lambda: e.copy_(p),
    }
    for fn in cases.values():
        for _ in range(5):
            fn()
    res = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            res[k] += timed(fn, reps)
    med = {k: statistics.median(t) for k, t in res.items()}
    per = {"ema_update": 12, "adam_step": 28, "ema_swap": 16, "copy (p -> e)": 8}
    print("flat buffer: %d elements, %.1f MB" % (n, n * 4 / 1e6))
    for k, t in res.items():
        print("%-14s median %7.1f us  min %7.1f  max %7.1f  (%d B/element: %.2f TB/s)   rounds: %s"
              % (k, med[k], min(t), max(t), per[k], per[k] * n / med[k] / 1e6, " ".join("%.1f" % u for u in t)), flush=True)
    yard = med["adam_step"] * 12 / 28
    print("yardstick: adam_step x 12 / 28 = %.1f us; ema_update / yardstick = %.3f; ema_update / adam_step = %.3f"
          % (yard, med["ema_update"] / yard, med["ema_update"] / med["adam_step"]))
    print(json.dumps({"mode": "kernel", "n": n, "median_us": med}))
    sys.exit(0)

# ---- mode == "step"
rounds, steps = num(1, 4), num(2, 40)
with_ema = "--no-ema" not in flags
if with_ema:
    from mdcv.optim import WeightEMA


def make(pipeline, ema_on):
    net = new_net()
    ema = WeightEMA(net, decay=0.9999, warmup=10) if ema_on else None
    opt = FusedAdam(net, lr=1e-3, pipeline=pipeline, **({"ema": ema} if ema_on else {}))

    def step():
        opt.zero_grad()
        loss = net(x, tg)[0].sum()
        loss.backward()
        opt.step()
        return loss
    for _ in range(6):
        step()
    return net, opt, ema, step


cases = {}
for pipeline in (False, True):
    for ema_on in ((False, True) if with_ema else (False,)):
        cases["pipeline=%d ema=%s" % (pipeline, "on " if ema_on else "off")] = make(pipeline, ema_on)
torch.cuda.synchronize()
res = {k: [] for k in cases}
for rnd in range(rounds):
    for name, (net, opt, ema, step) in cases.items():
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        res[name].append((time.perf_counter() - t0) / steps * 1e3)
for name, t in res.items():
    print("%-22s median %.3f ms  min %.3f  max %.3f  (%s)  %.0f img/s" % (name, statistics.median(t), min(t), max(t), " ".join("%.3f" % u for u in t),
                                                                          32 / statistics.median(t) * 1e3), flush=True)
print(json.dumps({"mode": "step", "tree": ROOT, "ema": with_ema, "median_ms": {k: statistics.median(t) for k, t in res.items()}}), flush=True)
if with_ema:
    a, b = cases["pipeline=0 ema=on "], cases["pipeline=1 ema=on "]
    groups = getattr(getattr(b[0], "_pipe_plan", None), "param_groups", None)
    same_p = torch.equal(a[0].flat_parameters()[0], b[0].flat_parameters()[0])
    same_e = torch.equal(a[2].shadow, b[2].shadow)
    print("full model after %d steps each: %s parameter groups; pipelined parameters == plain: %s; pipelined shadow == plain: %s; updates %d / %d; "
          "shadow finite: %s" % (6 + rounds * (steps + 3), len(groups) if groups else groups, same_p, same_e, a[2].updates, b[2].updates,
                                 bool(torch.isfinite(b[2].shadow).all())), flush=True)
