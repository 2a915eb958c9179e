"""Device-resident frame cache on the GPU (mdcv/data/framecache.py, the `_frames_` entry points of csrc/imgload.hip and csrc/imgaug.hip):
windows read in place out of a pool give Pillow's bytes, and loaders with `cache_bytes` give the batches of loaders without, bit for bit,
while each admitted file is decoded once.  Golden data only (tests/golden/imgload, tests/golden/imgaug)."""
import ctypes
import functools
import os
import sys
import warnings
from collections import Counter

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import imgaug_cases as K  # noqa: E402
import kptload_numpy as N  # noqa: E402

pytestmark = pytest.mark.gpu
ROWS = {"f0": (301, 173, 0.5, ["[20, 30, 40, 25]", "[150, 60, 70, 45]", "[260, 120, 50, 38]", "[5, 5, 160, 290]"]),
        "f1": (97, 211, 0.5, ["[10, 20, 60, 30]", "[50, 150, 40, 40]"]),
        "f2": (257, 129, 0.25, ["[30, 10, 100, 60]", "[200, 80, 40, 50]", "[120, 60, 20, 20]"]),
        "f3": (120, 90, 0.3, [])}                                     # tests/golden/imgload/dataset.csv without its skipped row
PATCHES = {"f0": 6, "f1": 2, "f2": 1, "f3": 2}                        # at 64 x 64, tile-and-scale


def _r(n):
    return (n + 255) // 256 * 256


def _check(got, u8, what):
    """tests/test_gpu_imgload.py's rule: 0 differing bytes before /255, exact fp32 after it"""
    want = torch.from_numpy(np.moveaxis(u8, -1, 0).astype(np.float32) / np.float32(255))
    got = got.cpu()
    assert got.shape == want.shape, what
    back = torch.round(got * 255).to(torch.uint8).numpy()
    assert int((back != np.moveaxis(u8, -1, 0)).sum()) == 0, what
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), what


def _imgload_cases():
    z = np.load(os.path.join(K.GL, "cases.npz"))
    out = []
    for i in range(int(z["n"])):
        fi, ts, patch, flip, bw, W, H = (int(v) for v in z[f"c{i}_params"])
        out.append(dict(i=i, name=K.NAMES[fi], ts=bool(ts), patch=patch, flip=bool(flip), W=W, H=H, scale=float(z[f"c{i}_scale"]),
                        u8=z[f"c{i}_u8"], jitter=None, affine=None, empty=K.NAMES[fi] == "f3"))
    return out


def _pool_of(frames, lead=13, gap=7):
    """frames back to back in one pool behind `lead` bytes, `gap` bytes apart (odd offsets, nothing aligned), the LAST frame ending on
    the pool's last byte; the filler is 0xEE, which no fixture's border would give -> (pool on the device, offsets)"""
    parts, offsets, at = [np.full(lead, 0xEE, np.uint8)], [], lead
    for k, f in enumerate(frames):
        offsets.append(at)
        parts.append(np.ascontiguousarray(f).reshape(-1))
        at += f.size
        if k + 1 < len(frames):
            parts.append(np.full(gap, 0xEE, np.uint8))
            at += gap
    return torch.from_numpy(np.concatenate(parts)).cuda(), offsets


def _kernel_names(fn):
    from mdcv import _lib
    L = _lib.lib()
    torch.cuda.synchronize()
    L.profile_begin()
    out = fn()
    torch.cuda.synchronize()
    names = []
    for i in range(L.profile_stop()):
        ms, buf = ctypes.c_float(), ctypes.create_string_buffer(256)
        L.profile_read(i, ctypes.byref(ms), buf, 256)
        names.append(buf.value.decode())                              # "(anonymous namespace)::imgload_hpass_kernel(int const*, ...)"
    return out, names


# ------------------------------------------------------------------------------------------------------------ 1. golden through the pool
def test_every_imgload_fixture_is_bit_exact_read_in_place():
    from mdcv.data import images as I
    frs = K.frames()
    seen = set()
    for c in _imgload_cases():
        g = K.geometry(I, c, frs)
        f = frs[c["name"]]
        pool, (off,) = _pool_of([f])
        assert off % 2 == 1 and off + f.size == pool.numel()          # odd offset; the frame ends on the pool's last byte
        imgs = I.transform_batch([None], [g], bw=c["u8"].shape[2] == 1, pool=pool, offsets=[off])
        _check(imgs[0], c["u8"], (c["i"], c["name"], c["ts"], c["patch"]))
        seen.add((c["ts"], g.window[0] > 0 or g.window[1] > 0, (3 * f.shape[1]) % 4 != 0))
    assert (True, True, True) in seen and any(not ts for ts, _, _ in seen)     # a window off the origin in a frame of odd pitch; border taps


def test_every_imgaug_fixture_is_bit_exact_read_in_place():
    from mdcv.data import images as I
    frs = K.frames()
    for c in K.cases()[0]:
        g = K.geometry(I, c, frs)
        f = frs[c["name"]]
        pool, (off,) = _pool_of([f], lead=1)
        imgs = I.transform_batch([None], [g], bw=c["u8"].shape[2] == 1, pool=pool, offsets=[off])
        _check(imgs[0], c["u8"], (c["i"], c["name"], c["jitter"], c["affine"]))


def test_a_batch_mixing_pooled_and_staged_images_is_one_launch_sequence():
    from mdcv.data import images as I
    frs = K.frames()
    for cs, want in ((_imgload_cases(), ["imgload_hpass", "imgload_vpass"]),
                     (K.cases()[0], ["imgload_hpass", "imgaug_patch_u8", "imgaug_jitter_stats", "imgaug_apply"])):
        cs = [c for c in cs if (c["W"], c["H"]) == (64, 64) and c["u8"].shape[2] == 3]
        assert len({c["name"] for c in cs}) >= 3 and len({c["ts"] for c in cs}) == 2
        geoms = [K.geometry(I, c, frs) for c in cs]
        pool, offs = _pool_of([frs[n] for n in K.NAMES])
        where = dict(zip(K.NAMES, offs))
        offsets = [where[c["name"]] if b % 3 != 1 else None for b, c in enumerate(cs)]       # every third image is staged
        assert None in offsets and len({o for o in offsets if o is not None}) >= 3
        imgs, names = _kernel_names(lambda: I.transform_batch([frs[c["name"]] for c in cs], geoms, pool=pool, offsets=offsets))
        assert len(names) == len(want) and all(w in n for w, n in zip(want, names)), names
        for b, c in enumerate(cs):
            _check(imgs[b], c["u8"], (b, c["i"], offsets[b]))


# ------------------------------------------------------------------------------------------------------------------ 6. bad references
def test_bad_frame_references_are_rejected_before_any_launch():
    from mdcv import _lib
    from mdcv.data import images as I
    frs = K.frames()
    c = [c for c in K.cases()[0] if c["ts"] and c["jitter"] and c["affine"] and (c["W"], c["H"]) == (64, 64) and c["u8"].shape[2] == 3
         and c["name"] == "f0"][0]
    g = K.geometry(I, c, frs)
    x0, y0, w, h = g.window
    assert (x0 > 0 or y0 > 0) and w > 0 and h > 0
    f = frs["f0"]
    pool, (off,) = _pool_of([f])
    pitch = 3 * f.shape[1]
    end = off + (y0 + h - 1) * pitch + 3 * (x0 + w)                   # one past the window's last byte
    good = (off, pitch, x0, y0)
    p = I.pack_layout([g], [0], 0, [good])
    host = np.zeros(p.nbytes, np.uint8)
    I.pack_batch(host, p, [g], [None], frefs=[good])
    L = _lib.lib()
    dev = torch.from_numpy(host).cuda()
    base = dev.data_ptr()
    out = torch.empty(1, 3, 64, 64, device="cuda")
    ws = torch.empty(int(L.imgload_workspace_bytes(1, p.max_scr_w, p.max_scr_h)), dtype=torch.uint8, device="cuda")
    aws = torch.empty(int(L.imgaug_workspace_bytes(1, 64, 64)), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    desc, aug = host[:I.DESC * 4].view(np.int32), host[p.aug_off:p.aug_off + I.AUG_DESC * 4].view(np.int32)

    def run(ref=good, pool_bytes=pool.numel(), augmented=False, d=desc, fref_host=True):
        r = np.array(ref, np.int64)
        d = np.ascontiguousarray(d, np.int32)
        rh = r.ctypes.data if fref_host else None
        src = (base + p.pix_off, 0, pool.data_ptr(), pool_bytes)
        if augmented:
            return L.imgload_aug_frames_batch(d.ctypes.data, base + p.desc_off, rh, base + p.fref_off, aug.ctypes.data, base + p.aug_off, 1,
                                              base + p.coef_off, p.n_coefs, *src, p.max_scr_w, p.max_scr_h, 3, 64, 64, ws.data_ptr(),
                                              aws.data_ptr(), out.data_ptr(), st)
        return L.imgload_frames_batch(d.ctypes.data, base + p.desc_off, rh, base + p.fref_off, 1, base + p.coef_off, p.n_coefs, *src,
                                      p.max_scr_w, p.max_scr_h, 3, 64, 64, ws.data_ptr(), out.data_ptr(), st)

    assert run(augmented=True) == 0 and run(augmented=True, pool_bytes=end) == 0         # to the byte
    torch.cuda.synchronize()
    _check(out[0], c["u8"], "valid")
    bad = dict(off_minus_2=dict(ref=(-2, pitch, x0, y0)), one_byte_past_the_pool=dict(pool_bytes=end - 1),
               off_past_the_pool=dict(ref=(off + 1 + pool.numel() - end, pitch, x0, y0)), pitch_one_short=dict(ref=(off, 3 * (x0 + w) - 1, x0, y0)),
               negative_x0=dict(ref=(off, pitch, -1, y0)), negative_y0=dict(ref=(off, pitch, x0, -1)),
               wrapping_product=dict(ref=(0, 1 << 62, 0, 4)), no_host_table=dict(fref_host=False), negative_pool=dict(pool_bytes=-1))
    for augmented in (False, True):
        for what, kw in bad.items():
            out.fill_(7.0)
            rc, names = _kernel_names(lambda: run(augmented=augmented, **kw))
            assert rc == -1 and names == [], (augmented, what, rc, names)
            assert float(out.min()) == 7.0 and float(out.max()) == 7.0, (augmented, what)     # nothing was enqueued
        d = desc.copy()
        d[7] = p.max_scr_w + 1                                        # the rest of the descriptor is checked as on the staged path
        assert run(augmented=augmented, d=d) == -1
        d = desc.copy()
        d[0] = 10 ** 6                                                # ... except word 0, which a pooled image does not use
        assert run(augmented=augmented, d=d) == 0
    # a staged row in the table answers as the staged entry point does: this descriptor has no staged bytes behind it
    assert run(ref=I.STAGED) == -1 and L.imgload_batch(desc.ctypes.data, base + p.desc_off, 1, base + p.coef_off, p.n_coefs, base + p.pix_off,
                                                       0, p.max_scr_w, p.max_scr_h, 3, 64, 64, ws.data_ptr(), out.data_ptr(), st) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- the image loader
def _csv(tmp_path, sizes=None, names=("f0", "f1", "f2", "f3")):
    lines = ["Name,URL,Width,Height,Scale,X0,Y0,H0,W0", "header,,,,,,,,"]
    for n in names:
        w, h, s, boxes = ROWS[n]
        w, h = (sizes or {}).get(n, (w, h))
        lines.append(",".join([f"{n}.png", "", str(w), str(h), str(s)] + [f'"{b}"' for b in boxes]))
    path = os.path.join(str(tmp_path), "set.csv")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def _epochs(csv_path, epochs=3, **kw):
    """every batch of `epochs` epochs (held on the device, as a trainer that lags would), the decode count per file, the statistics"""
    from mdcv.data import images as I
    frs, calls = K.frames(), Counter()

    def decode(p):
        name = os.path.splitext(os.path.basename(p))[0]
        calls[name] += 1
        return frs[name]

    kw = dict(dict(ts=True, bw=False, lr_flip=True, data_aug=True, shuffle=True, seed=3, batch_size=4, num_workers=4, prefetch=True), **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ld = I.ImageLabelBatches(csv_path, "", 64, 64, decode=decode, **kw)
    got = [[(list(u), x, t) for u, x, t in ld] for _ in range(epochs)]
    torch.cuda.synchronize()
    stats = ld.cache_stats()
    ld.close()
    assert ld.cache_stats() is None or ld.cache_stats()["pool_bytes"] == 0
    return got, calls, stats


def _same(a, b, what):
    assert len(a) == len(b) > 0
    for e, (ea, eb) in enumerate(zip(a, b)):
        assert len(ea) == len(eb) > 0
        for bi, ((ua, xa, ta), (ub, xb, tb)) in enumerate(zip(ea, eb)):
            assert ua == ub, (what, e, bi)
            assert torch.equal(xa, xb) and torch.equal(ta, tb), (what, e, bi)
            assert torch.equal(xa.view(torch.int32), xb.view(torch.int32)), (what, e, bi)


@functools.lru_cache(maxsize=None)
def _uncached(csv_path, ts, bw):
    return _epochs(csv_path, ts=ts, bw=bw, prefetch=True)


@pytest.mark.parametrize("prefetch", [True, False])
@pytest.mark.parametrize("bw", [False, True])
@pytest.mark.parametrize("ts", [True, False])
def test_three_epochs_equal_the_cacheless_loader_and_decode_each_file_once(tmp_path_factory, ts, bw, prefetch):
    csv_path = _csv(tmp_path_factory.getbasetemp())
    want, calls0, none = _uncached(csv_path, ts, bw)
    got, calls, st = _epochs(csv_path, ts=ts, bw=bw, prefetch=prefetch, cache_bytes=1 << 20)
    _same(got, want, (ts, bw, prefetch))                              # the fill epoch and both hit epochs
    per = PATCHES if ts else dict.fromkeys(PATCHES, 1)
    n = sum(per.values())
    assert none is None and calls0 == {k: 3 * v for k, v in per.items()}             # without: every sample, every epoch
    assert calls == dict.fromkeys(per, 1)                                             # with: every file once
    assert st["fills"] == 4 and st["hits"] == 3 * n - 4 and st["misses"] == dict(not_admitted=0, size_mismatch=0)
    assert st["fills"] + sum(st["misses"].values()) == sum(calls.values())
    assert st["bytes_reserved"] == st["pool_bytes"] == sum(_r(3 * w * h) for w, h, _, _ in ROWS.values())
    if ts:
        assert any(len(set(u)) < len(u) for e in got for u, _, _ in e)               # two patches of one frame in one batch


def test_partial_budget_mixes_both_kinds_in_one_batch_with_the_same_launches(tmp_path):
    from mdcv.data import images as I
    csv_path = _csv(tmp_path)
    budget = _r(3 * 301 * 173) + _r(3 * 120 * 90)                     # f0 and f3 fit; f1 and f2, between them in the file, do not
    kw = dict(shuffle=False, prefetch=False)                          # batch 1 is f0, f0, f1, f1, and statistics move batch by batch
    want, _, _ = _epochs(csv_path, **kw)
    got, calls, st = _epochs(csv_path, cache_bytes=budget, **kw)
    _same(got, want, "partial")
    assert calls == dict(f0=1, f1=6, f2=3, f3=1) and st["fills"] == 2 and st["hits"] == 3 * 8 - 2
    assert st["misses"] == dict(not_admitted=9, size_mismatch=0) and st["pool_bytes"] == st["bytes_reserved"] == budget
    frs = K.frames()

    def second_batch(**extra):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ld = I.ImageLabelBatches(csv_path, "", 64, 64, ts=True, lr_flip=True, data_aug=True, seed=3, batch_size=4, num_workers=1,
                                     decode=lambda p: frs[os.path.splitext(os.path.basename(p))[0]], **kw, **extra)
        it = iter(ld)
        next(it)
        before = ld.cache_stats()
        batch, names = _kernel_names(lambda: next(it))
        after = ld.cache_stats()
        it.close()
        ld.close()
        return batch, names, before, after
    (u0, x0, t0), names0, _, _ = second_batch()
    (u1, x1, t1), names1, b, a = second_batch(cache_bytes=budget)
    assert u0 == u1 == ["f0.png", "f0.png", "f1.png", "f1.png"] and torch.equal(x0, x1) and torch.equal(t0, t1)
    assert a["hits"] - b["hits"] == 2 and a["misses"]["not_admitted"] - b["misses"]["not_admitted"] == 2      # both kinds, one batch
    assert names1 == names0 and len(names1) in (3, 4) and "imgload_hpass" in names1[0], (names0, names1)       # the same kernels, no more


def test_a_file_whose_decode_differs_from_the_csv_is_never_cached(tmp_path):
    csv_path = _csv(tmp_path, sizes=dict(f1=(97, 210)))               # the CSV is wrong about f1; both loaders plan from the decode
    want, calls0, _ = _epochs(csv_path)
    got, calls, st = _epochs(csv_path, cache_bytes=1 << 20)
    _same(got, want, "mismatch")
    assert calls == dict(f0=1, f1=3 * PATCHES["f1"], f2=1, f3=1) and calls0["f1"] == calls["f1"]
    assert st["fills"] == 3 and st["misses"] == dict(not_admitted=0, size_mismatch=6) and st["hits"] == 3 * 11 - 3 - 6


# ------------------------------------------------------------------------------------------------------------------ 8. mini train step
def test_mini_darknet_step_fed_from_a_hit_epoch(tmp_path):
    from mdcv.yolo.models import Darknet
    csv_path = _csv(tmp_path)
    kw = dict(data_aug=False, epochs=2)
    want, _, _ = _epochs(csv_path, **kw)
    got, calls, st = _epochs(csv_path, cache_bytes=1 << 20, **kw)
    assert calls == dict.fromkeys(PATCHES, 1) and st["hits"] == 2 * 11 - 4
    mini = os.path.join(K.GOLDEN, "mini")
    losses = []
    for _, x, t in (got[1][0], want[1][0]):                           # epoch 1: every sample of the cached loader is a hit
        cwd = os.getcwd()
        os.chdir(mini)
        try:
            net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32")
            net.load_weights("mini.weights", net.get_start_weight_dim())
        finally:
            os.chdir(cwd)
        net = net.cuda().train()
        out = net(x, t)
        out[0].sum().backward()
        losses.append(float(out[0].detach()))
    assert np.isfinite(losses[0]) and losses[0] == losses[1], losses


# ------------------------------------------------------------------------------------------------------------------------ 7. key points
SHAPES = ((13, 9), (131, 97), (160, 160), (80, 80), (40, 1), (47, 49), (13, 9))


def _crop_epochs(batch_size=3, epochs=2, **kw):
    from mdcv.data import ConeCropBatches
    crops = [N.make_crop(h, w, 100 * i + 80) for i, (h, w) in enumerate(SHAPES)]
    labels = [N.make_label(h, w, 100 * i + 80) for i, (h, w) in enumerate(SHAPES)]
    names = [f"crop_{i}.png" for i in range(len(crops))]
    names[-1] = names[0]                                              # the first file once more, in another batch
    labels[-1] = labels[0]
    table = {os.path.join("mem", n): c for n, c in zip(names, crops)}
    calls = Counter()

    def decode(p):
        calls[p] += 1
        return table[p]
    if "cache_bytes" in kw:
        kw["probe"] = lambda p: table[p].shape[1::-1]
    ld = ConeCropBatches(names, labels, "mem", 80, batch_size, decode=decode, num_workers=4, **kw)
    got = []
    for e in range(epochs):
        with _LaunchCount() as lc:
            got.append([b for b in ld])
        assert lc.names == ["kptload"] * len(ld), lc.names             # one launch per batch, whatever the batch mixes
    torch.cuda.synchronize()
    st = ld.cache_stats()
    ld.close()
    return got, calls, st


class _LaunchCount:
    def __enter__(self):
        from mdcv import _lib
        self.L = _lib.lib()
        torch.cuda.synchronize()
        self.L.profile_begin()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.names = []
        for i in range(self.L.profile_stop()):
            ms, buf = ctypes.c_float(), ctypes.create_string_buffer(256)
            self.L.profile_read(i, ctypes.byref(ms), buf, 256)
            self.names.append("kptload" if "kptload" in buf.value.decode() else buf.value.decode())


def _same_crops(a, b, what):
    assert len(a) == len(b) > 0
    for e, (ea, eb) in enumerate(zip(a, b)):
        assert len(ea) == len(eb) > 0
        for bi, (x, y) in enumerate(zip(ea, eb)):
            for k in range(3):                                        # images, heat-maps (NaN positions included), points
                np.testing.assert_array_equal(x[k].cpu().numpy(), y[k].cpu().numpy(), err_msg=str((what, e, bi, k)))
                assert torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)), (what, e, bi, k)
            assert x[3] == y[3] and all(torch.equal(s, t) for s, t in zip(x[4], y[4])), (what, e, bi)


@pytest.mark.parametrize("prefetch", [True, False])
def test_key_point_batches_equal_the_cacheless_loader(prefetch):
    want, calls0, none = _crop_epochs(prefetch=prefetch)
    assert none is None and sum(calls0.values()) == 2 * len(SHAPES)                   # without: every sample, every epoch
    got, calls, st = _crop_epochs(prefetch=prefetch, cache_bytes=1 << 20)
    _same_crops(got, want, "all cached")
    files = len(SHAPES) - 1
    assert set(calls.values()) == {1} and len(calls) == files                          # with: every file once
    assert st["fills"] == files and st["hits"] == 2 * len(SHAPES) - files and st["misses"] == dict(not_admitted=0, size_mismatch=0)
    assert st["bytes_reserved"] == sum(_r(3 * h * w) for h, w in SHAPES[:-1]) and st["pool_bytes"] > st["bytes_reserved"]
    # a tiny budget: the two 13 x 9 crops and the 40 x 1 one fit, the full batches mix pooled and staged crops, still one launch each
    got, calls, st = _crop_epochs(prefetch=prefetch, cache_bytes=_r(3 * 13 * 9) + _r(3 * 40))
    _same_crops(got, want, "tiny budget")
    assert st["fills"] == 2 and st["hits"] == 2 * 3 - 2 and st["misses"] == dict(not_admitted=2 * 4, size_mismatch=0)
    assert calls[os.path.join("mem", "crop_0.png")] == 1 and calls[os.path.join("mem", "crop_4.png")] == 1
    assert calls[os.path.join("mem", "crop_1.png")] == 2
