"""Rates of the real-image loader (mdcv.data.ImageLabelBatches, csrc/imgload.hip) on one GPU.

(a) the device transform alone: ms per B=32 batch of 416x416 outputs from pre-decoded, pre-staged 1920x1080-class frames
    (LANCZOS tile-and-scale at scale 0.5 / 1.0 / 1.5; BILINEAR pad-and-resize of a frame of 1920s x 1080s for the same s)
(b) the whole loader with decode, img/s on 1 / 8 / 16 decode threads, PNG and JPEG files written to a temporary directory
(c) ms per YOLOv3 416x416 B=32 bf16 train step fed by the loader (plain, and with data_aug=True) against the same step fed by SyntheticCones
(d) the augmented transform (csrc/imgaug.hip) alone, B=32 of 416x416 from 1920x1080 frames, tile-and-scale at scale 1.0: no augmentation
    (the two-launch path), affine only, jitter + affine as data_aug draws them; each row several times over to show the run-to-run spread

(e) the frame cache (`cache_bytes`): the step of (c) fed without the cache, in the cache's fill epoch and in hit epochs, beside
    SyntheticCones on the same lease; staged bytes per batch with and without; the hit-epoch loader alone (img/s, host ms per batch)
(f) the blur / noise / contrast / sharpen launch (csrc/imgfx.hip) alone on a B=32 batch of 416x416: no flag (a copy), each op on
    every image, all four on every image at the largest radius the reference draws, and the four as the loader draws them

Device events after a warm-up, profiler off.  usage: loader_probe.py [files per format (default 32)] [parts, default abcd]"""
import contextlib
import ctypes
import io
import os
import random
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from mdcv.data import images as I  # noqa: E402
from mdcv.data.synth import SyntheticCones  # noqa: E402

B, S = 32, 416
NFILES = int(sys.argv[1]) if len(sys.argv) > 1 else 32
PARTS = sys.argv[2] if len(sys.argv) > 2 else "abcd"


def frame(seed, w=1920, h=1080):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([x * 255 // w, y * 255 // h, (x + y) % 256], -1).astype(np.int16)
    img += rng.integers(-12, 13, img.shape, dtype=np.int16)
    return np.clip(img, 0, 255).astype(np.uint8)


def ev_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def part_a(frames):
    print("(a) device transform alone, B=32 outputs of 416x416 RGB (ms per batch, kernel pair only; staged bytes per batch)")
    rng = random.Random(0)
    for filt in ("lanczos", "bilinear"):
        for s in (0.5, 1.0, 1.5):
            geoms, wins = [], []
            for b in range(B):
                f = frames[b % len(frames)]
                if filt == "lanczos":
                    n = I.n_patches(f.shape[1], f.shape[0], s, S, S)
                    g = I.sample_geometry(f.shape[1], f.shape[0], S, S, True, s, rng.randrange(n), b % 2)
                else:
                    w, h = int(1920 * s), int(1080 * s)
                    f = np.ascontiguousarray(np.resize(f, (h, w, 3)))
                    g = I.sample_geometry(w, h, S, S, False, 1.0, 0, b % 2)
                geoms.append(g)
                wins.append(I.crop_window(f, g))
            p = I.pack_layout(geoms, [w.nbytes for w in wins], 0)
            host = np.zeros(p.nbytes, np.uint8)
            I.pack_batch(host, p, geoms, wins)
            dev = torch.from_numpy(host).cuda()
            st = torch.cuda.current_stream()
            ms = ev_ms(lambda: I.launch_batch(dev, host, p, 3, S, S, st), 50)
            print(f"    {filt:8s} scale {s:3.1f}: {ms:7.3f} ms/batch  ({1e3 * B / ms:8.0f} img/s)  staged {p.nbytes / 2**20:6.2f} MiB "
                  f"(ksize {geoms[0].desc[3]}, scratch {p.max_scr_w}x{p.max_scr_h})")


def write_dataset(tmp, frames, fmt):
    from PIL import Image
    rng = random.Random(1)
    rows = ["Name,URL,Width,Height,Scale,X0,Y0,H0,W0", "header"]

    def save(i):
        Image.fromarray(frames[i % len(frames)]).save(os.path.join(tmp, f"{i}.{fmt}"), quality=90) if fmt == "jpg" else \
            Image.fromarray(frames[i % len(frames)]).save(os.path.join(tmp, f"{i}.{fmt}"), compress_level=1)
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(save, range(NFILES)))
    for i in range(NFILES):
        boxes = []
        for _ in range(rng.randint(1, 8)):
            w, h = rng.randint(10, 60), rng.randint(15, 90)
            boxes.append(f'"[{rng.randint(0, 1920 - w)}, {rng.randint(0, 1080 - h)}, {h}, {w}]"')
        rows.append(",".join([f"{i}.{fmt}", "", "1920", "1080", "1.0"] + boxes))
    path = os.path.join(tmp, f"train_{fmt}.csv")
    with open(path, "w") as f:
        f.write("\n".join(rows) + "\n")
    return path


def part_b(tmp, csvs):
    print("(b) whole loader with decode, 416x416 tile-and-scale at scale 1.0, B=32 (img/s; decode alone on the same threads)")
    from PIL import Image
    for fmt, path in csvs.items():
        files = [os.path.join(tmp, f"{i}.{fmt}") for i in range(NFILES)]
        for t in (1, 8, 16):
            frames_timed = 5 * B                       # as many frames as the loader run below decodes in its timed batches
            with ThreadPoolExecutor(t) as ex:
                list(ex.map(lambda p: np.asarray(Image.open(p).convert("RGB")), files[:B]))
                t0 = time.perf_counter()
                list(ex.map(lambda i: np.asarray(Image.open(files[i % NFILES]).convert("RGB")), range(frames_timed)))
                dec = frames_timed / (time.perf_counter() - t0)
            ld = I.ImageLabelBatches(path, tmp, S, S, ts=True, lr_flip=True, batch_size=B, num_workers=t)
            it = iter(ld)
            next(it)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for k, (_, imgs, tg) in enumerate(it):
                n += imgs.shape[0]
                if k == 4:
                    break
            torch.cuda.synchronize()
            rate = n / (time.perf_counter() - t0)
            ld.close()
            print(f"    {fmt:4s} {t:2d} threads: loader {rate:7.0f} img/s   decode alone {dec:7.0f} frames/s")


def part_c(tmp, csv_path, steps=10):
    print(f"(c) YOLOv3 416x416 B=32 bf16 train step (ms/step over {steps} steps after 3 warm-up steps)")
    from mdcv.optim import FusedAdam
    from mdcv.yolo.models import Darknet
    d = tempfile.mkdtemp()
    cfg = bench.write_yolo_cfg(d, classes=1)
    cwd = os.getcwd()
    os.chdir(d)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        net = Darknet(cfg, 2.0, 1.6, 25.0, 0.1, True, precision="bf16").cuda().train()
    os.chdir(cwd)
    opt = FusedAdam(net, lr=1e-4)

    def run(data):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i, (_, x, tg) in enumerate(data):
            if i == 3:
                s.record()
            opt.zero_grad()
            out = net(x, tg)
            out[0].sum().backward()
            opt.step()
            if i == 3 + steps - 1:
                e.record()
                break
        e.synchronize()
        return s.elapsed_time(e) / steps

    syn = run(SyntheticCones(B, S, S, 16, 1, batches=steps + 4, seed=3))
    for t in (16, 8):
        ld = I.ImageLabelBatches(csv_path, tmp, S, S, ts=True, lr_flip=False, batch_size=B, num_workers=t)
        real = run(ld)
        ld.close()
        print(f"    SyntheticCones: {syn:7.2f} ms/step   ImageLabelBatches (JPEG, {t:2d} threads): {real:7.2f} ms/step")
    ld = I.ImageLabelBatches(csv_path, tmp, S, S, ts=True, lr_flip=True, batch_size=B, num_workers=16, data_aug=True)
    real = run(ld)
    ld.close()
    print(f"    SyntheticCones: {syn:7.2f} ms/step   ImageLabelBatches (JPEG, 16 threads, data_aug): {real:7.2f} ms/step")


def part_e(tmp, csv_path, steps=10):
    print(f"(e) frame cache: YOLOv3 416x416 B=32 bf16 train step, JPEG, 16 threads, shuffle (ms/step over {steps} steps after 3 warm-up "
          f"steps; the fill epoch from its first batch)")
    from mdcv.optim import FusedAdam
    from mdcv.yolo.models import Darknet
    d = tempfile.mkdtemp()
    cfg = bench.write_yolo_cfg(d, classes=1)
    cwd = os.getcwd()
    os.chdir(d)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        net = Darknet(cfg, 2.0, 1.6, 25.0, 0.1, True, precision="bf16").cuda().train()
    os.chdir(cwd)
    opt = FusedAdam(net, lr=1e-4)

    def run(data, warm=3):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if warm == 0:
            s.record()
        for i, (_, x, tg) in enumerate(data):
            if i == warm and warm:
                s.record()
            opt.zero_grad()
            out = net(x, tg)
            out[0].sum().backward()
            opt.step()
            if i == warm + steps - 1:
                e.record()
                break
        e.synchronize()
        return s.elapsed_time(e) / steps

    staged = []
    layout = I.pack_layout

    def recording_layout(*a, **k):
        p = layout(*a, **k)
        staged.append(p.nbytes)
        return p
    I.loader.pack_layout = recording_layout                  # where the loader looks it up
    try:
        syn = run(SyntheticCones(B, S, S, 16, 1, batches=steps + 4, seed=3))
        ld = I.ImageLabelBatches(csv_path, tmp, S, S, ts=True, lr_flip=False, batch_size=B, num_workers=16)
        assert len(ld) >= steps + 3, "more files: an epoch must hold the timed steps"
        plain = run(ld)
        ld.close()
        plain_mib = np.mean(staged) / 2**20
        ld = I.ImageLabelBatches(csv_path, tmp, S, S, ts=True, lr_flip=False, batch_size=B, num_workers=16, cache_bytes=64 << 30)
        fill = run(ld, warm=0)
        fill_stats = ld.cache_stats()
        del staged[:]
        hits = [run(ld) for _ in range(3)]
        hit_mib = np.mean(staged) / 2**20
        syn2 = run(SyntheticCones(B, S, S, 16, 1, batches=steps + 4, seed=4))
        print(f"    SyntheticCones {syn:7.2f} ms/step (again at the end: {syn2:7.2f})   no cache {plain:7.2f} ms/step   "
              f"fill epoch {fill:7.2f} ms/step   hit epochs " + " / ".join(f"{h:.2f}" for h in hits) + " ms/step")
        print(f"    staged per batch: {plain_mib:7.3f} MiB without the cache, {hit_mib:7.3f} MiB in a hit epoch; after the fill epoch's "
              f"{steps} steps: {fill_stats}")
        times = []
        stage = ld._stage

        def timed_stage(*a):
            t0 = time.perf_counter()
            r = stage(*a)
            times.append(time.perf_counter() - t0)
            return r
        ld._stage = timed_stage
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(x.shape[0] for _, x, _ in ld)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"    hit-epoch loader alone ({len(ld)} batches, 16 threads): {n / dt:7.0f} img/s; host staging (plan, labels, packing) "
              f"{1e3 * np.mean(times):6.2f} ms/batch")
        print(f"    {ld.cache_stats()}")
        ld.close()
    finally:
        I.loader.pack_layout = layout


def part_d(frames, repeats=5):
    print("(d) augmented transform alone, B=32 outputs of 416x416 RGB from 1920x1080 frames, tile-and-scale at scale 1.0 "
          f"(ms per batch, kernels only; {repeats} timings of 50 batches each)")
    patch_mb = B * S * S * 4 / 1e6                           # one pass over the uint8 RGBX patches
    out_mb = B * 3 * S * S * 4 / 1e6
    for name, jit_on, aff_on in (("none (two launches)", False, False), ("affine only", False, True), ("jitter + affine", True, True)):
        geoms, wins = [], []
        for b in range(B):
            f = frames[b % len(frames)]
            rng = random.Random(f"probe/{b}")
            g = I.sample_geometry(f.shape[1], f.shape[0], S, S, True, 1.0, rng.randrange(I.n_patches(f.shape[1], f.shape[0], 1.0, S, S)), b % 2)
            aug = I.draw_augmentation(rng, jit_on, aff_on)
            if aug.affine is not None:
                aug.matrix = I.inverse_affine_matrix(S, S, *aug.affine)
            g.aug = aug if aug else None
            geoms.append(g)
            wins.append(I.crop_window(f, g))
        p = I.pack_layout(geoms, [w.nbytes for w in wins], 0)
        host = np.zeros(p.nbytes, np.uint8)
        I.pack_batch(host, p, geoms, wins)
        dev = torch.from_numpy(host).cuda()
        st = torch.cuda.current_stream()
        ms = sorted(ev_ms(lambda: I.launch_batch(dev, host, p, 3, S, S, st), 50) for _ in range(repeats))
        n_jit = sum(g.aug is not None and g.aug.jitter is not None for g in geoms)
        # bytes the augmentation adds: the patch written once, read by the statistics pass (jittered images) and by the apply pass
        moved = patch_mb * (2 + n_jit / B) + out_mb if p.aug else 0.0
        print(f"    {name:20s}: median {ms[len(ms) // 2]:7.3f} ms/batch  min {ms[0]:7.3f}  max {ms[-1]:7.3f}   jittered {n_jit:2d}/{B}"
              + (f"   patch + output traffic {moved:6.1f} MB" if p.aug else ""))
        L = I._lib.lib()                                         # one more batch under the in-library profiler: each kernel's own time
        torch.cuda.synchronize()
        L.profile_begin()
        I.launch_batch(dev, host, p, 3, S, S, st)
        torch.cuda.synchronize()
        for i in range(L.profile_stop()):
            t, buf = ctypes.c_float(), ctypes.create_string_buffer(256)
            L.profile_read(i, ctypes.byref(t), buf, 256)
            name = buf.value.decode().split("::")[-1].split("(")[0]
            print(f"        {name:32s} {1e3 * t.value:8.1f} us")


def part_f(repeats=5):
    print(f"(f) imgfx launch alone, B=32 of 416x416 RGB fp32 in and out, {2 * B * 3 * S * S * 4 / 1e6:.1f} MB read + written "
          f"(ms per batch; {repeats} timings of 50 launches each, then the kernel's own time from one profiled launch)")
    L = I._lib.lib()
    src = (torch.randint(0, 256, (B, 3, S, S), device="cuda").float() / 255.0).contiguous()
    dst = torch.empty_like(src)
    st = torch.cuda.current_stream()

    def drawn(b):
        rng = random.Random(f"probe/{b}")
        return I.draw_imgfx(rng, lambda: random.Random(f"probe/{b}/imgaug"), True, True, True, True)
    rows = (("no flag (copy)", lambda b: None), ("blur sigma 1.0 (r 2)", lambda b: I.ImageFx(blur=1.0)),
            ("blur sigma 2.99 (r 4)", lambda b: I.ImageFx(blur=2.99)), ("noise, per pixel", lambda b: I.ImageFx(noise=(4.0, False, b))),
            ("noise, per channel", lambda b: I.ImageFx(noise=(4.0, True, b))), ("contrast", lambda b: I.ImageFx(contrast=(7, 0.6))),
            ("sharpen", lambda b: I.ImageFx(sharpen=0.3)),
            ("all four, r 4, per channel", lambda b: I.ImageFx(2.99, (4.0, True, b), (7, 0.6), 0.3)), ("as the loader draws them", drawn))
    for name, make in rows:
        fxs = [make(b) for b in range(B)]
        desc, luts = [], []
        for fx in fxs:
            desc.append(I.fx_descriptor(fx, len(luts)))
            if fx and fx.contrast is not None:
                luts.append(I.sigmoid_table(*fx.contrast))
        desc = np.stack(desc).astype(np.int32)
        ddev = torch.from_numpy(desc).cuda()
        ldev = torch.from_numpy(np.stack(luts)).cuda() if luts else None

        def run():
            L.check(L.imgfx_batch(desc.ctypes.data, ddev.data_ptr(), B, ldev.data_ptr() if ldev is not None else None, len(luts), 3, S, S,
                                  src.data_ptr(), dst.data_ptr(), st.cuda_stream), "imgfx_batch")
        ms = sorted(ev_ms(run, 50) for _ in range(repeats))
        torch.cuda.synchronize()
        L.profile_begin()
        run()
        torch.cuda.synchronize()
        t = ctypes.c_float()
        for i in range(L.profile_stop()):
            L.profile_read(i, ctypes.byref(t), ctypes.create_string_buffer(256), 256)
        flags = [sum(getattr(fx, k) is not None for fx in fxs if fx) for k in ("blur", "noise", "contrast", "sharpen")]
        print(f"    {name:28s}: median {ms[len(ms) // 2]:7.3f} ms/batch  min {ms[0]:7.3f}  max {ms[-1]:7.3f}   kernel {1e3 * t.value:7.1f} us"
              f"   images with blur / noise / contrast / sharpen: {flags}")


def main():
    torch.cuda.set_device(0)
    if "f" in PARTS:
        part_f()
    if not set(PARTS) & set("abcde"):
        return
    frames = [frame(i) for i in range(8)]
    if "a" in PARTS:
        part_a(frames)
    if "d" in PARTS:
        part_d(frames)
    if "b" in PARTS or "c" in PARTS or "e" in PARTS:
        with tempfile.TemporaryDirectory() as tmp:
            csvs = {fmt: write_dataset(tmp, frames, fmt) for fmt in (("png", "jpg") if "b" in PARTS else ("jpg",))}
            if "b" in PARTS:
                part_b(tmp, csvs)
            if "c" in PARTS:
                part_c(tmp, csvs["jpg"])
            if "e" in PARTS:
                part_e(tmp, csvs["jpg"])


if __name__ == "__main__":
    main()
