"""What the cone pose solver costs.

    pnp_cost.py [reps]
        1. mdcv_cone_pnp alone at M = 64 and 1024 cones (seeded poses of the default cone at 2.5..10 m, tilts of +-15 degrees, 0.5 px noise,
           three cameras, windows), max_iters 30 and 100: device events around `reps` back-to-back launches, five windows each after a
           warm-up; median and all windows; the longest refinement (accepted steps) is read once behind the windows.
        2. end to end: `FrameConeDetector.detect_frames` over 16 frames (the four golden frames, four times) on the mini models with and
           without a camera, a host clock around whole calls that end in the detector's own synchronisation, alternating, five windows each."""
import os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdcv import _lib
from mdcv.rektnet.keypoint_net import KeypointNet
from mdcv.rektnet.pose import cone_model, synthetic_cones
from mdcv.yolo.detect import FrameConeDetector
from mdcv.yolo.models import Darknet

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
dev = torch.device("cuda", 0)
CAMS = np.array([[1200.0, 1200.0, 640.0, 360.0], [1150.0, 1210.0, 600.0, 380.0], [900.0, 880.0, 512.0, 300.0]])
model = cone_model()


def cones(M):
    c = synthetic_cones(M, CAMS, 38, 0.5, True)
    return [torch.from_numpy(c[k]).to(dev) for k in ("pts", "window", "owner")]


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def clock(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n * 1e6


def report(what, paths, measure, n, after):
    for fn in paths.values():
        measure(fn, 5)
    res = {k: [] for k in paths}
    for _ in range(5):
        for name, fn in paths.items():
            res[name].append(measure(fn, n))
    for name, t in res.items():
        paths[name]()
        print("%-24s %-22s median %9.1f us (%s)  %s" % (what, name, statistics.median(t), " ".join("%.1f" % v for v in t), after()), flush=True)


L, st = _lib.pnp_lib(), torch.cuda.current_stream(dev).cuda_stream
cam_d, mod_d = torch.from_numpy(CAMS).to(dev), torch.from_numpy(model).to(dev)
for M in (64, 1024):
    pts, win, own = cones(M)
    pose, info = torch.empty(M, 16, dtype=torch.float64, device=dev), torch.empty(M, 4, dtype=torch.int32, device=dev)

    def solve(iters):
        return lambda: L.check(L.cone_pnp(pts.data_ptr(), win.data_ptr(), own.data_ptr(), cam_d.data_ptr(), 3, mod_d.data_ptr(), M, iters,
                                          pose.data_ptr(), info.data_ptr(), st), "cone_pnp")
    report("cone_pnp alone, M %d" % M, {"max_iters 30": solve(30), "max_iters 100": solve(100)}, window, reps,
           lambda: "longest refinement %d steps, at the cap %d" % (int(info[:, 1:3].max()), int((info[:, 0] == 32).sum())))

cwd = os.getcwd()
os.chdir(os.path.join(ROOT, "tests", "golden", "mini"))
net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32")
net.load_weights("mini.weights", net.get_start_weight_dim())
os.chdir(cwd)
net = net.to(dev).eval()
torch.manual_seed(7)
kp = KeypointNet(7, (80, 80), precision="fp32").to(dev).eval()
z = np.load(os.path.join(ROOT, "tests", "golden", "imgload", "frames.npz"))
frames = [np.ascontiguousarray(z[k]) for k in sorted(z.files)] * 4
dets = {"camera=None": FrameConeDetector(net, kp, conf_thres=0.05), "camera=(fx, fy, cx, cy)": FrameConeDetector(net, kp, conf_thres=0.05, camera=CAMS[0])}
seen = []
report("detect_frames, 16, mini", {k: (lambda det=det: seen.append(sum(int(r.has_crop.sum()) for r in det.detect_frames(frames)))) for k, det in dets.items()},
       clock, max(reps // 20, 5), lambda: "cones %d" % seen[-1])
