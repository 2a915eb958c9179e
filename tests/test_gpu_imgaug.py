"""Augmented real-image loader on the GPU (csrc/imgaug.hip, mdcv/data/images.py): ColorJitter and affine byte for byte against Pillow 12.2
(tests/golden/imgaug, written by tests/golden/make_golden_imgaug.py) and, where golden files would be too large, against the NumPy
restatement that tests/test_imgaug_host.py pins to Pillow."""
import ctypes
import os
import random
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import imgaug_cases as K  # noqa: E402
import imgaug_numpy as N  # noqa: E402

pytestmark = pytest.mark.gpu
BOX_TOL_PX = 2e-4          # tests/test_imgaug_host.py derives it


def _check(got, u8, what):
    """`out * 255` equals the uint8 image exactly, and out is the correctly rounded u8 / 255"""
    want = torch.from_numpy(np.moveaxis(u8, -1, 0).astype(np.float32) / np.float32(255))
    got = got.cpu()
    assert got.shape == want.shape, what
    back = torch.round(got * 255).to(torch.uint8).numpy()
    assert int((back != np.moveaxis(u8, -1, 0)).sum()) == 0, (what, int((back != np.moveaxis(u8, -1, 0)).sum()))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), what


def _kernel_names(L, fn):
    torch.cuda.synchronize()
    L.profile_begin()
    out = fn()
    torch.cuda.synchronize()
    names = []
    for i in range(L.profile_stop()):
        ms, buf = ctypes.c_float(), ctypes.create_string_buffer(256)
        L.profile_read(i, ctypes.byref(ms), buf, 256)
        names.append(buf.value.decode())
    return out, names


def test_kernel_chain_matches_pillow_on_every_fixture():
    from mdcv.data import images as I
    frs = K.frames()
    cs, _ = K.cases()
    kinds = set()
    for c in cs:
        g = K.geometry(I, c, frs)
        imgs = I.transform_batch([frs[c["name"]]], [g], bw=c["u8"].shape[2] == 1)
        _check(imgs[0], c["u8"], (c["i"], c["name"], c["jitter"], c["affine"]))
        kinds.add((g.aug is not None and g.aug.jitter is not None, g.aug is not None and g.aug.affine is not None, c["u8"].shape[2], g.flip))
        if g.aug is not None and g.aug.jitter is not None:
            kinds.add(g.aug.jitter[0].index(I.CONTRAST))
    assert {0, 3} <= kinds and kinds & {1, 2}                    # contrast first, last, in the middle
    assert {(True, False, 3, False), (False, True, 3, False), (True, True, 3, True), (True, True, 1, True)} <= kinds


def test_mixed_batch_of_frames_augmented_and_box_free_in_one_launch_sequence():
    from mdcv import _lib
    from mdcv.data import images as I
    frs = K.frames()
    cs = [c for c in K.cases()[0] if (c["W"], c["H"]) == (64, 64) and c["u8"].shape[2] == 3]
    assert {c["name"] for c in cs} == set(K.NAMES) and len({c["ts"] for c in cs}) == 2
    geoms = [K.geometry(I, c, frs) for c in cs]
    assert any(g.aug is None for g in geoms) and any(g.aug is not None for g in geoms)
    imgs, names = _kernel_names(_lib.lib(), lambda: I.transform_batch([frs[c["name"]] for c in cs], geoms))
    assert len(names) == 4 and "imgload_hpass" in names[0] and "imgaug_patch_u8" in names[1] and "imgaug_jitter_stats" in names[2] \
        and "imgaug_apply" in names[3], names
    for b, c in enumerate(cs):
        _check(imgs[b], c["u8"], (b, c["i"]))
    # box-free samples come out as the two-launch path writes them, and a batch of affine-only samples needs no statistics pass
    plain = [g for g in geoms if g.aug is None]
    fr = [frs[c["name"]] for c, g in zip(cs, geoms) if g.aug is None]
    two, names = _kernel_names(_lib.lib(), lambda: I.transform_batch(fr, plain))
    assert len(names) == 2 and "imgload_vpass" in names[1], names
    k = 0
    for b, g in enumerate(geoms):
        if g.aug is None:
            assert torch.equal(imgs[b], two[k])
            k += 1
    aff = [(c, g) for c, g in zip(cs, geoms) if g.aug is not None and g.aug.jitter is None]
    _, names = _kernel_names(_lib.lib(), lambda: I.transform_batch([frs[c["name"]] for c, _ in aff], [g for _, g in aff]))
    assert len(names) == 3 and not any("jitter_stats" in n for n in names), names


def _big_batch(I, B=32, S=416, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:540, 0:960]
    frames, geoms, augs = [], [], []
    for b in range(B):
        f = np.stack([x * 255 // 960, y * 255 // 540, (x + y + 31 * b) % 256], -1).astype(np.int16)
        f += rng.integers(-20, 21, f.shape, dtype=np.int16)
        frames.append(np.clip(f, 0, 255).astype(np.uint8))
        r = random.Random(f"big/{b}")
        n = I.n_patches(960, 540, 1.0, S, S)
        aug = I.draw_augmentation(r, True, True) if b % 8 != 7 else None          # every eighth sample passes through
        if aug is not None and aug.affine is not None:
            aug.matrix = I.inverse_affine_matrix(S, S, *aug.affine)
        g = I.sample_geometry(960, 540, S, S, True, 1.0, r.randrange(n), b % 2)
        g.aug = aug if aug else None
        geoms.append(g)
    return frames, geoms


def _bare(I, g):
    return I.sample_geometry(g.frame[0], g.frame[1], g.width, g.height, g.ts, g.scale, g.patch_index, False)


@pytest.mark.parametrize("bw", [False, True])
def test_batch_of_32_at_416_equals_the_numpy_restatement(bw):
    from mdcv.data import images as I
    frames, geoms = _big_batch(I)
    assert sum(g.aug is not None and g.aug.jitter is not None for g in geoms) >= 8
    got = I.transform_batch(frames, geoms, bw=bw)
    patches = I.transform_batch(frames, [_bare(I, g) for g in geoms])        # the uint8 patches, from the path test_gpu_imgload.py pins
    patches = torch.round(patches * 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    for b, g in enumerate(geoms):
        a = g.aug
        want = N.augment(patches[b], a.jitter if a else None, a.matrix if a and a.affine else None, bw, g.flip)
        _check(got[b], want, (b, a.jitter if a else None, a.affine if a else None))


def test_hue_on_every_rgb_value():
    """all 2^24 colours as 64 patches of 512 x 512, pad-and-resize at the frame's own size (a copy), hue alone first in the chain with
    unit factors behind it (blends with alpha 1.0 are copies); shifts of both signs"""
    from mdcv.data import images as I
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([v & 255, (v >> 8) & 255, v >> 16], -1).astype(np.uint8).reshape(64, 512, 512, 3)
    for hue in (0.04, -0.0275):
        geoms = []
        for b in range(64):
            g = I.sample_geometry(512, 512, 512, 512, False)
            g.aug = I.Augmentation(((I.HUE, I.BRIGHTNESS, I.SATURATION, I.CONTRAST), (1.0, 1.0, 1.0), hue), None)
            geoms.append(g)
        got = I.transform_batch(list(rgb), geoms)
        got = torch.round(got * 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
        want = N.hue(rgb, hue)
        assert int((got != want).sum()) == 0, (hue, int((got != want).sum()))


def test_bad_descriptors_are_rejected():
    from mdcv import _lib
    from mdcv.data import images as I
    frs = K.frames()
    c = [c for c in K.cases()[0] if c["jitter"] and c["affine"] and (c["W"], c["H"]) == (64, 64) and c["u8"].shape[2] == 3 and not c["empty"]][0]
    g = K.geometry(I, c, frs)
    w = I.crop_window(frs[c["name"]], g)
    p = I.pack_layout([g], [w.nbytes], 0)
    host = np.zeros(p.nbytes, np.uint8)
    I.pack_batch(host, p, [g], [w])
    L = _lib.lib()
    dev = torch.from_numpy(host).cuda()
    out = torch.empty(1, 3, 64, 64, device="cuda")
    ws = torch.empty(int(L.imgload_workspace_bytes(1, p.max_scr_w, p.max_scr_h)), dtype=torch.uint8, device="cuda")
    assert L.imgaug_workspace_bytes(1, 64, 64) == 64 * 64 * 4 + 4
    assert L.imgaug_workspace_bytes(0, 64, 64) == -1 and L.imgaug_workspace_bytes(1, 4097, 4096) == -1
    aws = torch.empty(int(L.imgaug_workspace_bytes(1, 64, 64)), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    desc = host[:I.DESC * 4].view(np.int32)
    aug = host[p.aug_off:p.aug_off + I.AUG_DESC * 4].view(np.int32)

    def run(d=desc, a=aug, C=3, H=64, W=64, mw=p.max_scr_w, dbuf=dev, aw=aws):
        h, ha = np.ascontiguousarray(d, np.int32), np.ascontiguousarray(a, np.int32)
        base = dbuf.data_ptr()
        return L.imgload_aug_batch(h.ctypes.data, base + p.desc_off, ha.ctypes.data, base + p.aug_off, 1, base + p.coef_off, p.n_coefs,
                                   base + p.pix_off, p.src_bytes, mw, p.max_scr_h, C, H, W, ws.data_ptr(), aw.data_ptr() if aw is not None else None,
                                   out.data_ptr(), st)
    assert run() == 0
    torch.cuda.synchronize()
    _check(out[0], c["u8"], "valid")
    nan = np.array([np.nan], np.float64).view(np.int32)
    for field, value in ((12, 2), (12, -1), (13, 4), (14, int(aug[13])), (16, -1), (17, int(np.array([-0.5], np.float32).view(np.int32)[0])),
                         (18, int(np.array([np.nan], np.float32).view(np.int32)[0])), (19, int(np.array([np.inf], np.float32).view(np.int32)[0])),
                         (20, 256), (20, -1), (21, 2), (22, 1), (23, 7), (1, int(nan[1])), (11, int(np.array([np.inf], np.float64).view(np.int32)[1]))):
        a = aug.copy()
        a[field] = value
        assert run(a=a) == -1, (field, value)
    for field, value in ((0, p.src_bytes), (7, p.max_scr_w + 1), (17, 2), (18, 1)):       # the loader's own descriptor is still checked
        d = desc.copy()
        d[field] = value
        assert run(d=d) == -1, (field, value)
    assert run(C=2) == -1 and run(mw=p.max_scr_w - 1) == -1 and run(aw=None) == -1 and run(H=4097, W=4096) == -1
    # corrupted DEVICE copies (the host never sees them): zeros, no fault
    for off, field, value in ((p.aug_off, 13, 9), (p.aug_off, 21, 5), (p.aug_off, 3, int(nan[1])), (p.desc_off, 7, 10 ** 6), (p.desc_off, 17, 3)):
        bad = host.copy()
        bad[off:off + 4 * max(I.DESC, I.AUG_DESC)].view(np.int32)[field] = value
        out.fill_(7.0)
        assert run(dbuf=torch.from_numpy(bad).cuda()) == 0
        torch.cuda.synchronize()
        assert float(out.abs().max()) == 0.0, (off, field)
    out.fill_(7.0)
    assert run() == 0
    torch.cuda.synchronize()
    _check(out[0], c["u8"], "valid again")


def _loader(I, name, prefetch, workers=4, **kw):
    z = K.npz(name)
    frs = K.frames()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return z, I.ImageLabelBatches(os.path.join(K.GL, "dataset.csv"), "", int(z["W"]), int(z["H"]), ts=name == "loader_ts.npz",
                                      lr_flip=True, batch_size=int(z["B"]), shuffle=False, num_workers=workers, prefetch=prefetch,
                                      seed=int(z["seed"]), data_aug=True,
                                      decode=lambda p: frs[os.path.splitext(os.path.basename(p))[0]], **kw)


@pytest.mark.parametrize("name", ["loader_ts.npz", "loader_pad.npz"])
@pytest.mark.parametrize("prefetch", [True, False])
def test_data_aug_loader_equals_the_golden_batches(name, prefetch):
    from mdcv.data import images as I
    z, ld = _loader(I, name, prefetch)
    B, n, W, H = int(z["B"]), len(z["files"]), int(z["W"]), int(z["H"])
    tol = torch.tensor([0, BOX_TOL_PX / W, BOX_TOL_PX / H, BOX_TOL_PX / W, BOX_TOL_PX / H], dtype=torch.float64)
    count = 0
    for e in range(3):                                       # the loader draws epoch e's augmentation itself: seed / epoch / index
        for bi, (uris, imgs, tg) in enumerate(ld):
            sl = slice(bi * B, min(n, (bi + 1) * B))
            assert imgs.is_cuda and tg.is_cuda and imgs.dtype == torch.float32 and tg.dtype == torch.float32
            for b in range(imgs.shape[0]):
                _check(imgs[b], z[f"e{e}_u8"][sl][b], (name, e, bi, b))
            want = torch.from_numpy(z[f"e{e}_targets"][sl])
            assert ((tg.cpu().double() - want.double()).abs() <= tol).all(), (name, e, bi)
            count += imgs.shape[0]
    assert count == 3 * n
    ld.close()


def test_two_runs_with_one_seed_are_bit_identical():
    from mdcv.data import images as I
    runs = []
    for prefetch in (True, False):
        _, ld = _loader(I, "loader_ts.npz", prefetch, workers=8 if prefetch else 1)
        ld.shuffle = True
        got = []
        for e in range(2):
            for _, imgs, tg in ld:
                got.append((imgs.clone(), tg.clone()))
        runs.append(got)
        ld.close()
    assert len(runs[0]) == len(runs[1]) > 0
    for (a, ta), (b, tb) in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ta.view(torch.int32), tb.view(torch.int32))


def test_mini_darknet_step_fed_by_the_augmented_loader():
    from mdcv.data import images as I
    from mdcv.yolo.models import Darknet
    z, ld = _loader(I, "loader_ts.npz", True)
    uris, imgs, tg = next(iter(ld))
    ld.close()
    B = int(z["B"])
    x_ref = torch.from_numpy(np.moveaxis(z["e0_u8"][:B], -1, 1).astype(np.float32) / np.float32(255))
    assert torch.equal(imgs.cpu(), x_ref)
    assert any(K.unpack_aug(v) != (None, None) for v in z["e0_aug"][:B])
    mini = os.path.join(K.GOLDEN, "mini")
    losses = []
    for x, t in ((imgs, tg), (x_ref.cuda(), tg.clone())):
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
