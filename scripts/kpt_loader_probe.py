"""Rates of the key-point crop loader (mdcv.data.ConeCropBatches, csrc/kptload.hip) on one GPU.

(a) the kernel alone: us per B=256 batch of 80x80 outputs from pre-decoded, pre-staged crops of mixed sizes between 24 and 160 px, from
    device events (several timings of 200 launches each), beside its byte floor; one more launch under the in-library profiler
(b) the whole loader with the default decoder (PNG crops written to a temporary directory), img/s on 1 / 8 / 16 decode threads
(c) ms per KeypointNet + CrossRatioLoss + FusedAdam bf16 B=256 train step fed by the loader against the same step fed by SyntheticConeCrops
(d) the crop cache (`cache_bytes`): the whole loader of (b) without it, in its fill epoch and in hit epochs, and the step of (c)
    fed from hit epochs

usage: kpt_loader_probe.py [files (default 1024)] [parts, default abc]"""
import ctypes
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdcv.data import crops as C  # noqa: E402
from mdcv.data.synth import SyntheticConeCrops  # noqa: E402

B, S = 256, 80
NFILES = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
PARTS = sys.argv[2] if len(sys.argv) > 2 else "abc"
HBM_TBS = 5.2                                              # what the box sustains (`peaks` in bench.py's result line)
KP = np.array([[0.5, 0.04], [0.36, 0.36], [0.64, 0.36], [0.25, 0.66], [0.75, 0.66], [0.12, 0.96], [0.88, 0.96]])


def crop(seed):
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(24, 161)), int(rng.integers(24, 161))
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([x * 255 // w, y * 255 // h, (x + y) % 256], -1).astype(np.int16)
    img += rng.integers(-12, 13, img.shape, dtype=np.int16)
    label = np.clip(KP + rng.uniform(-0.02, 0.02, (7, 2)), 0, 0.999) * (w, h)
    return np.clip(img, 0, 255).astype(np.uint8), label


def ev_us(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return 1e3 * s.elapsed_time(e) / iters


def part_a(samples, repeats=5):
    crops, labels = [c for c, _ in samples[:B]], [l for _, l in samples[:B]]
    hots = [C.hot_pixels(l, c.shape[0], c.shape[1], "probe") for c, l in zip(crops, labels)]
    pts = [C.scale_points(l, c.shape[0], c.shape[1], S) for c, l in zip(crops, labels)]
    p = C.pack_layout([c.shape[:2] for c in crops])
    host = np.zeros(p.nbytes, np.uint8)
    C.pack_batch(host, p, crops, hots, pts)
    dev = torch.from_numpy(host).cuda()
    L = C._lib.lib()
    imgs = torch.empty(B, 3, S, S, device="cuda")
    hm = torch.empty(B, 7, S, S, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def run():                                             # the C entry alone: no allocation in the timed loop
        L.kptload_batch(host.ctypes.data + p.desc_off, dev.data_ptr() + p.desc_off, B, dev.data_ptr() + p.pix_off, p.src_bytes, S,
                        imgs.data_ptr(), hm.data_ptr(), st)

    us = sorted(ev_us(run, 200) for _ in range(repeats))
    out_mb = B * 10 * S * S * 4 / 1e6
    floor = out_mb / HBM_TBS                                # MB / (TB/s) = us
    print(f"(a) kernel alone, B={B} S={S}, crops 24..160 px ({p.src_bytes / 1e6:.2f} MB of pixels in, {out_mb:.1f} MB out): "
          f"median {us[len(us) // 2]:.1f} us/batch  min {us[0]:.1f}  max {us[-1]:.1f}   (back-to-back launches, events)")
    print(f"    byte floor {floor:.1f} us at {HBM_TBS} TB/s -> median / floor = {us[len(us) // 2] / floor:.2f}")
    torch.cuda.synchronize()
    L.profile_begin()
    run()
    torch.cuda.synchronize()
    for i in range(L.profile_stop()):
        t, buf = ctypes.c_float(), ctypes.create_string_buffer(256)
        L.profile_read(i, ctypes.byref(t), buf, 256)
        print(f"    one dispatch, its own begin/end: {buf.value.decode().replace('(anonymous namespace)::', '').split('(')[0]:24s} {1e3 * t.value:8.1f} us")


def write_dataset(tmp, samples):
    from PIL import Image

    def save(i):
        Image.fromarray(samples[i][0]).save(os.path.join(tmp, f"{i}.png"), compress_level=1)
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(save, range(len(samples))))
    return [f"{i}.png" for i in range(len(samples))], [l for _, l in samples]


def part_b(tmp, names, labels):
    from PIL import Image
    print(f"(b) whole loader with the default decoder, PNG crops, B={B} S={S} (img/s; decode alone on the same threads)")
    files = [os.path.join(tmp, n) for n in names]
    for t in (1, 8, 16):
        with ThreadPoolExecutor(t) as ex:
            t0 = time.perf_counter()
            list(ex.map(lambda f: np.asarray(Image.open(f).convert("RGB")), files))
            dec = len(files) / (time.perf_counter() - t0)
        ld = C.ConeCropBatches(names, labels, tmp, S, B, num_workers=t)
        for _ in ld:                                        # warm-up epoch: pinned buffers, file cache
            pass
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(b[0].shape[0] for b in ld)
        torch.cuda.synchronize()
        rate = n / (time.perf_counter() - t0)
        ld.close()
        print(f"    {t:2d} threads: loader {rate:8.0f} img/s   decode alone {dec:8.0f} img/s")


def part_c(tmp, names, labels, steps=10):
    from mdcv.optim import FusedAdam
    from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss
    from mdcv.rektnet.keypoint_net import KeypointNet
    print(f"(c) KeypointNet 80x80 B={B} bf16 train step (ms/step over {steps} steps after 3 warm-up steps)")
    torch.manual_seed(0)
    kp = KeypointNet(7, (S, S), precision="bf16").cuda().train()
    crit = CrossRatioLoss("l1_softargmax", True, 0.05, 0.05)
    opt = FusedAdam(kp, lr=1e-3)

    def run(data):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        i = 0
        while i < 3 + steps:
            for x, hm_t, pts_t, _, _ in data:
                if x.shape[0] != B:
                    continue
                if i == 3:
                    s.record()
                opt.zero_grad()
                hm, pts = kp(x)
                crit(hm, pts, hm_t, pts_t)[2].backward()
                opt.step()
                i += 1
                if i == 3 + steps:
                    break
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / steps

    syn = run(SyntheticConeCrops(B, S, batches=steps + 4, seed=3))
    for t in (16, 8):
        ld = C.ConeCropBatches(names, labels, tmp, S, B, num_workers=t)
        real = run(ld)
        ld.close()
        print(f"    SyntheticConeCrops: {syn:6.2f} ms/step ({1e3 * B / syn:7.0f} img/s)   ConeCropBatches (PNG, {t:2d} threads): "
              f"{real:6.2f} ms/step ({1e3 * B / real:7.0f} img/s)")


def part_d(tmp, names, labels, steps=10):
    print(f"(d) crop cache, PNG crops, B={B} S={S}, 16 threads (whole-loader img/s per epoch)")

    def epoch(ld):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(b[0].shape[0] for b in ld)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)
    ld = C.ConeCropBatches(names, labels, tmp, S, B, num_workers=16)
    plain = [epoch(ld) for _ in range(3)]
    ld.close()
    t0 = time.perf_counter()
    ld = C.ConeCropBatches(names, labels, tmp, S, B, num_workers=16, cache_bytes=1 << 30)
    built = time.perf_counter() - t0
    cached = [epoch(ld) for _ in range(4)]
    print("    no cache: " + " / ".join(f"{r:.0f}" for r in plain) + " img/s   cache: fill epoch " + f"{cached[0]:.0f}, hit epochs "
          + " / ".join(f"{r:.0f}" for r in cached[1:]) + f" img/s   (constructor with the header probe of {len(names)} files: {built:.2f} s)")
    print(f"    {ld.cache_stats()}")
    from mdcv.optim import FusedAdam
    from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss
    from mdcv.rektnet.keypoint_net import KeypointNet
    torch.manual_seed(0)
    kp = KeypointNet(7, (S, S), precision="bf16").cuda().train()
    crit = CrossRatioLoss("l1_softargmax", True, 0.05, 0.05)
    opt = FusedAdam(kp, lr=1e-3)

    def run(data):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        i = 0
        while i < 3 + steps:
            for x, hm_t, pts_t, _, _ in data:
                if x.shape[0] != B:
                    continue
                if i == 3:
                    s.record()
                opt.zero_grad()
                hm, pts = kp(x)
                crit(hm, pts, hm_t, pts_t)[2].backward()
                opt.step()
                i += 1
                if i == 3 + steps:
                    break
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / steps
    syn = run(SyntheticConeCrops(B, S, batches=steps + 4, seed=3))
    hit = run(ld)
    ld.close()
    print(f"    KeypointNet bf16 step: SyntheticConeCrops {syn:6.2f} ms/step ({1e3 * B / syn:7.0f} img/s)   cached ConeCropBatches, hit epochs: "
          f"{hit:6.2f} ms/step ({1e3 * B / hit:7.0f} img/s)")


def main():
    torch.cuda.set_device(0)
    samples = [crop(i) for i in range(max(NFILES, B))]
    if "a" in PARTS:
        part_a(samples)
    if "b" in PARTS or "c" in PARTS or "d" in PARTS:
        with tempfile.TemporaryDirectory() as tmp:
            names, labels = write_dataset(tmp, samples[:NFILES])
            if "b" in PARTS:
                part_b(tmp, names, labels)
            if "c" in PARTS:
                part_c(tmp, names, labels)
            if "d" in PARTS:
                part_d(tmp, names, labels)


if __name__ == "__main__":
    main()
