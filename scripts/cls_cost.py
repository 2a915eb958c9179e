"""What the class loss of the YOLO head costs, on the benchmark's detector configuration: yolo_baseline 416x416, 80 classes,
B=32, T=16 label rows per image, bf16, one process.

    cls_cost.py kernel [reps]
        `mdcv_yolo_cls_loss` (two launches) and `mdcv_yolo_cls_grad` (one) alone on each of the three heads (13², 26², 52²), ce and bce,
        behind one `mdcv_yolo_head_train` that leaves the workspace they read: device events around `reps` back-to-back calls, five
        windows each; beside them `mdcv_yolo_head_grad`, the dense pass over the same dlogits plane, for scale.
    cls_cost.py step [rounds] [steps]
        the training step (forward, backward, FusedAdam) of three models with the same weights -- built without the keyword, with
        cls_loss=0 and with cls_loss=1 -- timed alternately for `rounds` rounds of `steps` steps.  The first two run the same plan, so
        their difference is the noise of the measurement; the third adds nine launches to the step."""
import os, statistics, sys, tempfile, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from mdcv import _lib
from mdcv.yolo.models import Darknet

mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
dev = torch.device("cuda", 0)
B, T, C, A = 32, 16, 80, 3
ANCHORS = [[10, 13], [16, 30], [33, 23], [30, 61], [62, 45], [59, 119], [116, 90], [156, 198], [373, 326]]


def targets(gen):
    tg = bench.synth_targets(B, T, gen)
    real = tg.sum(-1) > 0
    tg[..., 0][real] = torch.randint(0, C, (int(real.sum()),), generator=gen).float()      # class ids over all 80 classes
    return tg


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


def line(name, t):
    print("%-44s median %6.1f us (%s)" % (name, statistics.median(t), " ".join("%.1f" % v for v in t)), flush=True)


if mode == "kernel":
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    L, K = _lib.lib(), _lib.cls_lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    tg = targets(g).to(dev)
    for G, stride, sl in ((13, 32, slice(6, 9)), (26, 16, slice(3, 6)), (52, 8, slice(0, 3))):
        an = torch.tensor([(w / stride, h / stride) for w, h in ANCHORS[sl]], dtype=torch.float32, device=dev)
        lg = (torch.randn(B, G, G, 256, generator=g) * 2).to(torch.bfloat16).to(dev)
        dl = torch.empty_like(lg)
        ws = torch.zeros(int(L.yolo_head_workspace_bytes(B, A, G, G)), dtype=torch.uint8, device=dev)
        cws = torch.zeros(int(K.yolo_cls_workspace_bytes()), dtype=torch.uint8, device=dev)
        out7, cls_out, one = torch.zeros(7, device=dev), torch.zeros(1, device=dev), torch.ones(1, device=dev)
        geo = (B, T, A, C, G, G, 0.5)
        L.check(L.yolo_head_train(_lib.BF16, lg.data_ptr(), 256, dl.data_ptr(), 256, 256, tg.data_ptr(), an.data_ptr(), *geo, 2.0, 1.6, 0.1, 25.0,
                                  ws.data_ptr(), out7.data_ptr(), one.data_ptr(), s), "yolo_head_train")
        line(f"{G}x{G}  yolo_head_grad (dense, for scale)", timed(lambda: L.yolo_head_grad(
            _lib.BF16, lg.data_ptr(), 256, dl.data_ptr(), 256, 256, tg.data_ptr(), an.data_ptr(), *geo, 2.0, 1.6, 0.1, 25.0, ws.data_ptr(),
            one.data_ptr(), s), reps))
        for name, m in _lib.CLS_MODES.items():
            line(f"{G}x{G}  yolo_cls_loss {name} (2 launches)", timed(lambda: K.yolo_cls_loss(
                _lib.BF16, lg.data_ptr(), 256, tg.data_ptr(), an.data_ptr(), *geo, m, 1.0, ws.data_ptr(), cws.data_ptr(), out7.data_ptr(),
                cls_out.data_ptr(), s), reps))
            line(f"{G}x{G}  yolo_cls_grad {name} (1 launch)", timed(lambda: K.yolo_cls_grad(
                _lib.BF16, lg.data_ptr(), 256, dl.data_ptr(), 256, 256, tg.data_ptr(), an.data_ptr(), *geo, m, 1.0, ws.data_ptr(), one.data_ptr(), s),
                reps))
        torch.cuda.synchronize()
        print("   owned cells %d of %d; class err word %d" % (int((ws.view(torch.int32)[:B * A * G * G] >= 0).sum()), B * A * G * G,
                                                              int(cws.view(torch.int32)[_lib.CLS_ERR_WORD])), flush=True)
else:
    from mdcv.optim import FusedAdam
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 30
    tmp = tempfile.mkdtemp()
    cfg = bench.write_yolo_cfg(tmp, classes=C)
    g = torch.Generator().manual_seed(1000)
    x = torch.rand(B, 3, 416, 416, generator=g).to(dev)
    tg = targets(g).to(dev)

    def make(**kw):
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            torch.manual_seed(0)
            net = Darknet(cfg, 2.0, 1.6, 25.0, 0.1, True, precision="bf16", **kw)
        finally:
            os.chdir(cwd)
        net = net.to(dev).train()
        opt = FusedAdam(net, lr=1e-3)

        def run(n):
            for _ in range(n):
                opt.zero_grad()
                out = net(x, tg)
                out[0].sum().backward()
                opt.step()
            return out
        run(6)
        return net, run

    cases = {"no keyword": make(), "cls_loss=0": make(cls_loss=0.0), "cls_loss=1 ce": make(cls_loss=1.0), "cls_loss=1 bce": make(cls_loss=1.0, cls_mode="bce")}
    torch.cuda.synchronize()
    res = {k: [] for k in cases}
    for rnd in range(rounds):
        for name, (net, run) in cases.items():
            run(3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run(steps)
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / steps * 1e3)
    base = statistics.median(res["cls_loss=0"])
    for name, t in res.items():
        med = statistics.median(t)
        net = cases[name][0]
        print("%-16s median %.3f ms  min %.3f  (%s)  %+.2f %% of the cls_loss=0 step; loss_cls %s" % (
            name, med, min(t), " ".join("%.3f" % v for v in t), 100 * (med - base) / base,
            "-" if net.loss_cls is None else "%.4f" % float(net.loss_cls)), flush=True)
