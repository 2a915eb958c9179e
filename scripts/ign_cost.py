"""What the prediction-IoU ignore rule of the YOLO head costs, on the benchmark's detector configuration: yolo_baseline
416x416, 80 classes, B=32, T=16 label rows per image, bf16, one process.

    ign_cost.py kernel [reps]
        `mdcv_yolo_ign_loss` (mask kernel + finalize) and `mdcv_yolo_ign_grad` alone on each of the three heads (13², 26², 52²), behind
        one `mdcv_yolo_head_train` that leaves the workspace they read: device events around `reps` back-to-back calls, five windows
        each; beside them `mdcv_yolo_head_train` without a gradient (init, assignment, `yolo_loss_kernel`, finalize: the loss kernel
        reads the same logits plane) and `mdcv_yolo_head_grad`.  Half of the cells within one pixel of a label predict that label, so
        the mask is not empty.
    ign_cost.py step [rounds] [steps]
        the training step (forward, backward, FusedAdam) of three models with the same weights -- built without the keyword, with
        pred_ignore=0 and with pred_ignore=0.7 -- timed alternately for `rounds` rounds of `steps` steps.  The first two run the same
        plan, so their difference is the noise of the measurement; the third adds six launches to the step.
    ign_cost.py plain [rounds] [steps]
        the no-keyword model alone: runs on a checkout of the parent commit as well, for a comparison across two trees."""
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
    print("%-52s median %6.1f us (%s)" % (name, statistics.median(t), " ".join("%.1f" % v for v in t)), flush=True)


if mode == "kernel":
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    L, K = _lib.lib(), _lib.ign_lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    tg = bench.synth_targets(B, T, g)
    for G, stride, sl in ((13, 32, slice(6, 9)), (26, 16, slice(3, 6)), (52, 8, slice(0, 3))):
        an = torch.tensor([(w / stride, h / stride) for w, h in ANCHORS[sl]], dtype=torch.float32)
        z = torch.randn(B, G, G, 256, generator=g) * 2
        zv = z[..., :255].view(B, G, G, 3, 85)
        for b in range(B):                                    # every second cell within a pixel of a label's cell predicts that label
            for r in tg[b]:
                if float(r.sum()) <= 0:
                    continue
                gx, gy, gw, gh = float(r[1]) * G, float(r[2]) * G, float(r[3]) * G, float(r[4]) * G
                for j in range(max(int(gy) - 1, 0), min(int(gy) + 1, G - 1) + 1):
                    for i in range(max(int(gx) - 1, 0), min(int(gx) + 1, G - 1) + 1):
                        if (i + j) % 2:
                            continue
                        zv[b, j, i, :, 0] = torch.logit(torch.tensor(min(max(gx - i, 0.02), 0.98)))
                        zv[b, j, i, :, 1] = torch.logit(torch.tensor(min(max(gy - j, 0.02), 0.98)))
                        zv[b, j, i, :, 2], zv[b, j, i, :, 3] = torch.log(gw / an[:, 0]), torch.log(gh / an[:, 1])
        lg, an, tgd = z.to(torch.bfloat16).to(dev), an.to(dev), tg.to(dev)
        dl = torch.empty_like(lg)
        ws = torch.zeros(int(L.yolo_head_workspace_bytes(B, A, G, G)), dtype=torch.uint8, device=dev)
        iws = torch.zeros(int(K.yolo_ign_workspace_bytes(B, A, G, G)), dtype=torch.uint8, device=dev)
        out7, ign_out, one = torch.zeros(7, device=dev), torch.zeros(2, device=dev), torch.ones(1, device=dev)
        geo = (B, T, A, C, G, G, 0.5, 2.0, 1.6, 0.1, 25.0)
        head = lambda: L.yolo_head_train(_lib.BF16, lg.data_ptr(), 256, None, 0, 256, tgd.data_ptr(), an.data_ptr(), *geo, ws.data_ptr(),  # noqa: E731
                                         out7.data_ptr(), None, s)
        line(f"{G}x{G}  yolo_head_train, no gradient (4 launches)", timed(head, reps))
        # the ignore rule rewrites nN in the head workspace: every timed call is preceded by the head call that restores it
        pair = timed(lambda: (head(), K.yolo_ign_loss(_lib.BF16, lg.data_ptr(), 256, tgd.data_ptr(), an.data_ptr(), *geo[:6], 0.7, 25.0,
                                                      ws.data_ptr(), iws.data_ptr(), out7.data_ptr(), ign_out.data_ptr(), s)), reps)
        line(f"{G}x{G}  ... + yolo_ign_loss thr 0.7 (2 launches)", pair)
        line(f"{G}x{G}  yolo_head_grad (dense)", timed(lambda: L.yolo_head_grad(
            _lib.BF16, lg.data_ptr(), 256, dl.data_ptr(), 256, 256, tgd.data_ptr(), an.data_ptr(), *geo, ws.data_ptr(), one.data_ptr(), s), reps))
        line(f"{G}x{G}  yolo_ign_grad (1 launch)", timed(lambda: K.yolo_ign_grad(
            _lib.BF16, dl.data_ptr(), 256, 256, B, A, C, G, G, iws.data_ptr(), one.data_ptr(), s), reps))
        torch.cuda.synchronize()
        print("   cells %d, ignored %d, negatives left %d" % (B * A * G * G, int(ign_out[0]), int(ign_out[1])), flush=True)
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

    cases = {"no keyword": make()}
    if mode == "step":
        cases.update({"pred_ignore=0": make(pred_ignore=0.0), "pred_ignore=0.7": make(pred_ignore=0.7)})
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
    base = statistics.median(res["pred_ignore=0" if mode == "step" else "no keyword"])
    for name, t in res.items():
        med = statistics.median(t)
        ni = getattr(cases[name][0], "noobj_ignored", None)
        print("%-16s median %.3f ms  min %.3f  (%s)  %+.2f %%; ignored per head %s" % (
            name, med, min(t), " ".join("%.3f" % v for v in t), 100 * (med - base) / base,
            "-" if ni is None else ni[:, 0].tolist()), flush=True)
