"""What the box loss of the YOLO head costs, on the benchmark's detector configuration: yolo_baseline 416x416, 80 classes,
B=32, T=16 label rows per image, bf16, one process.

    box_cost.py kernel [reps]
        `mdcv_yolo_box_loss` (two launches) and `mdcv_yolo_box_grad` (one) alone on each of the three heads (13², 26², 52²), per mode,
        behind one `mdcv_yolo_head_train` that leaves the workspace they read: device events around `reps` back-to-back calls, five
        windows each; beside them `mdcv_yolo_head_grad`, the dense pass over the same dlogits plane, for scale.
    box_cost.py step [rounds] [steps]
        the training step (forward, backward, FusedAdam) of five models with the same weights -- built without the keyword, with
        box_loss=0 and with box_loss=1 in each mode -- timed alternately for `rounds` rounds of `steps` steps.  The first two run the
        same plan, so their difference is the noise of the measurement; the others add nine launches and a memset to the step."""
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
    L, K = _lib.lib(), _lib.box_lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    tg = bench.synth_targets(B, T, g).to(dev)
    for G, stride, sl in ((13, 32, slice(6, 9)), (26, 16, slice(3, 6)), (52, 8, slice(0, 3))):
        an = torch.tensor([(w / stride, h / stride) for w, h in ANCHORS[sl]], dtype=torch.float32, device=dev)
        lg = (torch.randn(B, G, G, 256, generator=g) * 2).to(torch.bfloat16).to(dev)
        dl = torch.empty_like(lg)
        ws = torch.zeros(int(L.yolo_head_workspace_bytes(B, A, G, G)), dtype=torch.uint8, device=dev)
        bws = torch.zeros(int(K.yolo_box_workspace_bytes()), dtype=torch.uint8, device=dev)
        out7, box_out, one = torch.zeros(7, device=dev), torch.zeros(2, device=dev), torch.ones(1, device=dev)
        geo = (B, T, A, C, G, G, 0.5)
        L.check(L.yolo_head_train(_lib.BF16, lg.data_ptr(), 256, dl.data_ptr(), 256, 256, tg.data_ptr(), an.data_ptr(), *geo, 2.0, 1.6, 0.1, 25.0,
                                  ws.data_ptr(), out7.data_ptr(), one.data_ptr(), s), "yolo_head_train")
        line(f"{G}x{G}  yolo_head_grad (dense, for scale)", timed(lambda: L.yolo_head_grad(
            _lib.BF16, lg.data_ptr(), 256, dl.data_ptr(), 256, 256, tg.data_ptr(), an.data_ptr(), *geo, 2.0, 1.6, 0.1, 25.0, ws.data_ptr(),
            one.data_ptr(), s), reps))
        for name, m in _lib.BOX_MODES.items():
            line(f"{G}x{G}  yolo_box_loss {name} (2 launches)", timed(lambda: K.yolo_box_loss(
                _lib.BF16, lg.data_ptr(), 256, tg.data_ptr(), an.data_ptr(), *geo, m, 1.0, ws.data_ptr(), bws.data_ptr(), out7.data_ptr(),
                box_out.data_ptr(), s), reps))
            line(f"{G}x{G}  yolo_box_grad {name} (1 launch)", timed(lambda: K.yolo_box_grad(
                _lib.BF16, lg.data_ptr(), 256, dl.data_ptr(), 256, 256, tg.data_ptr(), an.data_ptr(), *geo, m, 1.0, ws.data_ptr(), one.data_ptr(), s),
                reps))
        torch.cuda.synchronize()
        print("   owned cells %d of %d; mean IoU %.4f" % (int((ws.view(torch.int32)[:B * A * G * G] >= 0).sum()), B * A * G * G, float(box_out[1])),
              flush=True)
else:
    from mdcv.optim import FusedAdam
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 30
    tmp = tempfile.mkdtemp()
    cfg = bench.write_yolo_cfg(tmp, classes=C)
    g = torch.Generator().manual_seed(1000)
    x = torch.rand(B, 3, 416, 416, generator=g).to(dev)
    tg = bench.synth_targets(B, T, g).to(dev)

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

    cases = {"no keyword": make(), "box_loss=0": make(box_loss=0.0)}
    cases.update({"box_loss=1 " + m: make(box_loss=1.0, box_mode=m) for m in _lib.BOX_MODES})
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
    base = statistics.median(res["box_loss=0"])
    for name, t in res.items():
        med = statistics.median(t)
        net = cases[name][0]
        print("%-16s median %.3f ms  min %.3f  (%s)  %+.2f %% of the box_loss=0 step; loss_box %s box_iou %s" % (
            name, med, min(t), " ".join("%.3f" % v for v in t), 100 * (med - base) / base,
            "-" if net.loss_box is None else "%.4f" % float(net.loss_box), "-" if net.box_iou is None else "%.4f" % float(net.box_iou)), flush=True)
