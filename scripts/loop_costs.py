#!/usr/bin/env python3
"""Where the gap between bench.py's headline step and the reference's UNCHANGED training-loop statements comes from: the same model
and batch (YOLOv3 416^2, batch 32, bf16) stepped with the loop's three host-side habits switched on one at a time --
  stock torch.optim.Adam over model.parameters() (CVC-YOLOv3/train.py:180-187) instead of mdcv.optim.FusedAdam,
  the batch copied from pinned host memory every step (train.py:60-61),
  the sixteen blocking .item() / .to('cpu') reads per step (train.py:63, 75, 85-89).
Then the native loops beside them: mdcv.yolo.train.run_epoch over the same resident batch (one bookkeeping launch and one row copy per step, no
host read), the headline step three times for its spread, and the RektNet twin at batch 256 (headline step, the unchanged train_eval.py
statements, mdcv.rektnet.train.train_model).
usage: loop_costs.py [steps]"""
import os, sys, tempfile, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from mdcv.yolo.models import Darknet
from mdcv.optim import FusedAdam

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
dev = torch.device("cuda", 0)
tmp = tempfile.mkdtemp()
cfg = bench.write_yolo_cfg(tmp)
os.chdir(tmp)
g = torch.Generator().manual_seed(1000)
xh, th = torch.rand(32, 3, 416, 416, generator=g).pin_memory(), bench.synth_targets(32, 16, g).pin_memory()
xd, td = xh.to(dev), th.to(dev)


def run(name, optim, h2d, items, fused_kw=None):
    torch.manual_seed(0)
    net = Darknet(cfg, 2.0, 1.6, 25.0, 0.1, True).to(dev).train()
    if optim == "fused":
        opt = FusedAdam(net, lr=1e-3)
    else:
        opt = torch.optim.Adam(filter(lambda p: p.requires_grad, net.parameters()), lr=1e-3, weight_decay=0.0, **(fused_kw or {}))

    def step():
        imgs, targets = (xh.to(dev, non_blocking=True), th.to(dev, non_blocking=True)) if h2d else (xd, td)
        if items:
            n = ((targets[:, :, 1:5] > 0).sum(dim=2) > 1).sum().item() + 1e-12
        opt.zero_grad()
        losses = net(imgs, targets)
        losses[0].sum().backward()
        opt.step()
        if items:
            logged = [l.sum().to("cpu").item() for l in losses]
            tot = losses[0].item() / n
            t0 = losses[0].item()
            pct = [l.item() / t0 * 100 for l in losses[1:]]
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    print("%-78s %7.3f ms  %6.0f img/s" % (name, ms, 32 / ms * 1e3), flush=True)
    del net, opt
    torch.cuda.empty_cache()
    return ms


base = run("FusedAdam, resident batch, no host reads (bench.py's headline step)", "fused", False, False)
a = run("stock torch.optim.Adam (foreach), resident batch, no host reads", "stock", False, False)
a2 = run("stock torch.optim.Adam(fused=True), resident batch, no host reads", "stock", False, False, {"fused": True})
b = run("FusedAdam, batch from pinned host memory every step", "fused", True, False)
c = run("FusedAdam, resident batch, the loop's sixteen .item() reads", "fused", False, True)
d = run("stock Adam + host batch + .item() reads (the unchanged loop)", "stock", True, True)
e = run("FusedAdam + host batch + .item() reads", "fused", True, True)
print("optimizer %+.3f ms (fused=True: %+.3f) ; host batch %+.3f ms ; host reads %+.3f ms ; all three %+.3f ms" % (a - base, a2 - base, b - base, c - base, d - base))


# ---- the native loops
from mdcv.yolo.train import run_epoch
from mdcv.rektnet.train import train_model
from mdcv.rektnet.keypoint_net import KeypointNet
from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss


def report(name, ms, B):
    print("%-78s %7.3f ms  %6.0f img/s" % (name, ms, B / ms * 1e3), flush=True)
    return ms


def run_native_yolo(name):
    torch.manual_seed(0)
    net = Darknet(cfg, 2.0, 1.6, 25.0, 0.1, True).to(dev).train()
    opt = FusedAdam(net, lr=1e-3)
    batch = (["resident"] * 32, xd, td)
    lines, stats = [], {}
    run_epoch("train", [batch] * 5, 10 ** 9, opt, net, 0, 1, [0], log=lines.append)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_epoch("train", [batch] * steps, 10 ** 9, opt, net, 1, 1, [0], log=lines.append, stats=stats)      # returns behind its one wait: the sums are read
    ms = (time.perf_counter() - t0) / steps * 1e3
    assert len(lines) == 5 + steps + 2
    report(name + " [host waits: %d]" % stats["host_waits"], ms, 32)
    del net, opt
    torch.cuda.empty_cache()
    return ms


nat = run_native_yolo("native run_epoch: FusedAdam, resident batch, one log launch per step")
heads = [base] + [run("headline step again", "fused", False, False) for _ in range(2)]
print("headline spread over three runs: %.3f .. %.3f ms ; unchanged loop %.3f ms ; native run_epoch %.3f ms (%+.3f ms against the headline's mean)"
      % (min(heads), max(heads), d, nat, nat - sum(heads) / 3))

# RektNet, batch 256
RB = 256
g = torch.Generator().manual_seed(2000)
rxh, rph = torch.rand(RB, 3, 80, 80, generator=g).pin_memory(), (torch.rand(RB, 7, 2, generator=g) * (79 / 80)).pin_memory()
rhh = torch.zeros(RB, 7, 80, 80).pin_memory()
rxd, rpd, rhd = rxh.to(dev), rph.to(dev), rhh.to(dev)


def rekt_parts(stock):
    torch.manual_seed(0)
    kp = KeypointNet(7, (80, 80)).to(dev).train()
    crit = CrossRatioLoss("l1_softargmax", True, 0.05, 0.05)
    opt = torch.optim.Adam(kp.parameters(), lr=0.1) if stock else FusedAdam(kp, lr=0.1)
    return kp, crit, opt


def run_rekt(name, unchanged):
    kp, crit, opt = rekt_parts(unchanged)

    def step():
        if unchanged:                                            # train_eval.py:60-78
            x_batch, y_hm_batch, y_points_batch = rxh.to(dev), rhh.to(dev), rph.to(dev)
        else:
            x_batch, y_hm_batch, y_points_batch = rxd, rhd, rpd
        opt.zero_grad()
        output = kp(x_batch)
        loc_loss, geo_loss, loss = crit(output[0], output[1], y_hm_batch, y_points_batch)
        loss.backward()
        opt.step()
        if unchanged:
            loc_loss, geo_loss, loss = loc_loss.item(), geo_loss.item(), loss.item()
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return report(name, (time.perf_counter() - t0) / steps * 1e3, RB)


def run_native_rekt(name):
    kp, crit, opt = rekt_parts(False)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.999)
    batch = (rxd, rhd, rpd, ["resident"] * RB, None)
    val = [(rxd[:4], rhd[:4], rpd[:4], ["resident"] * 4, None)]
    marks = []
    # epoch 0 warms up; epoch 1 is timed from its "EPOCH 1" line to its "Training:" line, which is written behind the epoch's one wait
    train_model(kp, tmp, [batch] * steps, crit, opt, sched, 2, val, 10 ** 9, (80, 80), 7, False, [], "loop_costs", False,
                progress=lambda text: None, log=lambda line: marks.append((line, time.perf_counter())))
    t = {line.strip().split(":")[0]: at for line, at in marks[-2:]}
    return report(name, (t["Training"] - t["EPOCH 1"]) / steps * 1e3, RB)


rbase = [run_rekt("RektNet: FusedAdam, resident batch, no host reads (the headline step)", False) for _ in range(3)]
runch = run_rekt("RektNet: stock Adam + host batch + three .item() reads (the unchanged loop)", True)
rnat = run_native_rekt("RektNet: native train_model: FusedAdam, resident batch, one log launch per step")
print("RektNet headline spread over three runs: %.3f .. %.3f ms ; unchanged loop %.3f ms ; native train_model %.3f ms (%+.3f ms against the headline's mean)"
      % (min(rbase), max(rbase), runch, rnat, rnat - sum(rbase) / 3))
