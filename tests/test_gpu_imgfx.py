"""Blur / noise / contrast / sharpen on the GPU (csrc/imgfx.hip, mdcv/data/images.py): the kernel's floats bit for bit against the NumPy
restatement that tests/test_imgfx_host.py pins (tests/helpers/imgfx_numpy.py), the descriptor checks, and the loader with the four
options on against the restatement applied to the batches of the same loader with them off."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import imgaug_cases as K  # noqa: E402
import imgfx_numpy as N  # noqa: E402

pytestmark = pytest.mark.gpu
SIGMA = {2: 1.0, 4: 2.99, 7: 4.9}          # radius -> a sigma that gives it


def _image(H, W, seed):
    """random bytes; runs of 0 and 255 along every border, so that the reflected taps and both clips are exercised"""
    a = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    a[:3, : W // 2], a[-2:, W // 3:], a[:, :2], a[H // 2:, -3:] = 0, 255, 255, 0
    a[5:9, 7:30], a[H - 12:H - 8, 4:W - 4] = 255, 0
    return a


def _floats(u8):
    """[B,H,W,3] uint8 -> [B,3,H,W] fp32 holding u / 255, as the loader's kernels write it"""
    return np.ascontiguousarray(np.moveaxis(u8, -1, 1)).astype(np.float32) / np.float32(255)


def _pack(I, fxs):
    desc, luts = [], []
    for fx in fxs:
        desc.append(I.fx_descriptor(fx, len(luts)))
        if fx and fx.contrast is not None:
            luts.append(I.sigmoid_table(*fx.contrast))
    return np.stack(desc).astype(np.int32), (np.stack(luts) if luts else np.zeros((0, 256), np.uint8))


def _run(L, desc, luts, src, dst, dev_desc=None, C=3, H=None, W=None):
    B = len(desc)
    d = torch.from_numpy(desc if dev_desc is None else dev_desc).cuda()
    l = torch.from_numpy(luts).cuda() if len(luts) else None
    rc = L.imgfx_batch(desc.ctypes.data, d.data_ptr(), B, l.data_ptr() if l is not None else None, len(luts), C,
                       src.shape[2] if H is None else H, src.shape[3] if W is None else W, src.data_ptr(), dst.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _want(u8, fx):
    if fx is None:
        return u8
    return N.apply(u8, fx.blur, fx.noise, fx.contrast, fx.sharpen)


def _sets(I):
    F = I.ImageFx
    return {
        "alone": [F(blur=SIGMA[2]), F(noise=(6.5, False, 12345)), F(contrast=(7, 0.55)), F(sharpen=0.4),
                  F(SIGMA[7], (7.65, True, 0xFFFFFFFF), (10, 0.45), 0.5), None],
        "radii": [F(blur=SIGMA[4]), F(blur=SIGMA[7]), F(noise=(40.0, True, 7)), F(SIGMA[4], (3.0, False, 99), (5, 0.75), 0.11),
                  F(SIGMA[2], (0.7, True, 0), (8, 0.6), 0.25), F(blur=0.0005, sharpen=1.0)],
    }


@pytest.mark.parametrize("which", ["alone", "radii"])
@pytest.mark.parametrize("size", [(40, 48), (80, 96)])           # (H, W): below one 64 x 16 tile's width; 2 x 5 tiles with inner seams
def test_kernel_equals_the_restatement_bit_for_bit(size, which):
    from mdcv import _lib
    from mdcv.data import images as I
    H, W = size
    fxs = _sets(I)[which]
    assert [I.blur_radius(s) for s in SIGMA.values()] == list(SIGMA)
    u8 = np.stack([_image(H, W, 10 * H + b) for b in range(len(fxs))])
    desc, luts = _pack(I, fxs)
    src = torch.from_numpy(_floats(u8)).cuda()
    dst = torch.full_like(src, 7.0)
    assert _run(_lib.lib(), desc, luts, src, dst) == 0
    want = torch.from_numpy(_floats(np.stack([_want(u8[b], fx) for b, fx in enumerate(fxs)])))
    got = dst.cpu()
    for b, fx in enumerate(fxs):
        bad = int((torch.round(got[b] * 255) != torch.round(want[b] * 255)).sum())
        assert bad == 0, (which, size, b, bad)
        assert torch.equal(got[b].view(torch.int32), want[b].view(torch.int32)), (which, size, b)
        if fx is None:
            assert torch.equal(got[b].view(torch.int32), src[b].cpu().view(torch.int32))
        else:
            assert not torch.equal(got[b], src[b].cpu()) or fx.blur == 0.0005
    assert torch.equal(src.cpu(), torch.from_numpy(_floats(u8)))  # out of place: the input is left alone


def test_an_image_without_flags_is_copied_whatever_its_floats_are():
    from mdcv import _lib
    from mdcv.data import images as I
    desc, luts = _pack(I, [None, I.ImageFx(sharpen=0.0)])
    src = torch.rand(2, 3, 33, 70, device="cuda") * 3 - 1
    dst = torch.zeros_like(src)
    assert _run(_lib.lib(), desc, luts, src, dst) == 0
    assert torch.equal(dst[0].view(torch.int32), src[0].view(torch.int32))
    assert float(dst[1].min()) >= 0 and float(dst[1].max()) <= 1  # flagged: goes through the bytes


def test_bad_descriptors_are_rejected():
    from mdcv import _lib
    from mdcv.data import images as I
    L = _lib.lib()
    H, W = 40, 48
    fxs = [I.ImageFx(SIGMA[4], (3.0, True, 5), (6, 0.5), 0.3), I.ImageFx(contrast=(9, 0.7))]
    desc, luts = _pack(I, fxs)
    u8 = np.stack([_image(H, W, b) for b in range(2)])
    src = torch.from_numpy(_floats(u8)).cuda()
    dst = torch.full_like(src, 7.0)

    def untouched():
        return float(dst.min()) == 7.0 and float(dst.max()) == 7.0

    nan32, inf32 = (int(np.array([v], np.float32).view(np.int32)[0]) for v in (np.nan, np.inf))
    nan64 = np.array([np.nan], np.float64).view(np.int32)
    for field, value in ((2, int(desc[0, 2]) + 1),               # sum q != 256
                         (3, int(desc[0, 3]) + 1), (6, -2), (8, 1),   # ... a negative tap, a tap beyond the radius
                         (1, 8), (1, 0),                         # r = 8
                         (20, 1), (23, -1),                      # reserved words
                         (16, 2), (16, -1),                      # table index out of range
                         (0, 2), (10, -1), (11, 2), (15, 3), (17, 2), (18, nan32), (19, inf32), (14, int(nan64[1]))):
        d = desc.copy()
        d[0, field] = value
        assert _run(L, d, luts, src, dst) == -1 and untouched(), (field, value)
    n = src.numel()
    flat = torch.empty(2 * n, device="cuda")
    flat.fill_(7.0)
    stream = torch.cuda.current_stream().cuda_stream
    dd, ll = torch.from_numpy(desc).cuda(), torch.from_numpy(luts).cuda()
    for s_at, d_at in ((0, 0), (0, n - 1), (n - 1, 0)):          # dst overlapping src: the same buffer, the last float on either side
        rc = L.imgfx_batch(desc.ctypes.data, dd.data_ptr(), 2, ll.data_ptr(), 2, 3, H, W, flat.data_ptr() + 4 * s_at, flat.data_ptr() + 4 * d_at, stream)
        torch.cuda.synchronize()
        assert rc == -1 and float(flat.min()) == 7.0 and float(flat.max()) == 7.0, (s_at, d_at)
    assert _run(L, desc, luts, src, dst, C=1) == -1 and _run(L, desc, luts, src, dst, H=15) == -1 and _run(L, desc, luts, src, dst, W=15) == -1
    assert untouched()
    # a corrupted DEVICE copy (the host never sees it): that image is zeros, its neighbour is right, nothing faults
    for field, value in ((1, 9), (16, 5), (21, 1), (2, 255)):
        bad = desc.copy()
        bad[0, field] = value
        dst.fill_(7.0)
        assert _run(L, desc, luts, src, dst, dev_desc=bad) == 0
        assert float(dst[0].abs().max()) == 0.0, (field, value)
        assert torch.equal(dst[1].cpu(), torch.from_numpy(_floats(_want(u8[1], fxs[1])[None]))[0])
    dst.fill_(7.0)
    assert _run(L, desc, luts, src, dst) == 0
    assert torch.equal(dst.cpu(), torch.from_numpy(_floats(np.stack([_want(u8[b], fxs[b]) for b in range(2)]))))


def _loader(I, ts, fx_on, cache_bytes):
    frs = K.frames()
    W, H = (64, 64) if ts else (96, 64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return I.ImageLabelBatches(os.path.join(K.GL, "dataset.csv"), "", W, H, ts=ts, lr_flip=True, data_aug=True, batch_size=4, shuffle=False,
                                   num_workers=2, seed=7, blur=fx_on, noise=fx_on, contrast=fx_on, sharpen=fx_on, cache_bytes=cache_bytes,
                                   decode=lambda p: frs[os.path.splitext(os.path.basename(p))[0]])


@pytest.mark.parametrize("cache_bytes", [None, 1 << 20])
@pytest.mark.parametrize("ts", [True, False])
def test_loader_equals_the_restatement_of_its_own_plain_batches(ts, cache_bytes):
    from mdcv.data import images as I
    on, off = _loader(I, ts, True, cache_bytes), _loader(I, ts, False, cache_bytes)
    frs = K.frames()
    seen = set()
    for e in range(2):
        index = 0
        for (ua, a, ta), (ub, b, tb) in zip(on, off):
            assert ua == ub and a.shape == b.shape and a.data_ptr() != b.data_ptr()
            assert torch.equal(ta.view(torch.int32), tb.view(torch.int32))               # the earlier draws and the boxes are untouched
            base = torch.round(b * 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
            for k in range(a.shape[0]):
                size = frs[os.path.splitext(os.path.basename(ua[k]))[0]].shape[1::-1]
                g, h = on.plan(index, e, size), off.plan(index, e, size)
                assert h.fx is None and (g.patch_index, g.flip) == (h.patch_index, h.flip)
                want = torch.from_numpy(_floats(_want(base[k], g.fx)[None]))[0]
                assert torch.equal(a[k].cpu().view(torch.int32), want.view(torch.int32)), (ts, cache_bytes, e, index)
                if g.fx is not None:
                    seen |= {n for n in ("blur", "noise", "contrast", "sharpen") if getattr(g.fx, n) is not None}
                else:
                    seen.add("none")
                index += 1
        assert index == len(on.img_files)
    assert seen == {"blur", "noise", "contrast", "sharpen", "none"}
    if cache_bytes is not None:
        assert on.cache_stats()["hits"] > 0
    on.close()
    off.close()


def test_the_fx_launch_runs_only_for_a_batch_with_a_flag():
    import ctypes
    from mdcv import _lib
    from mdcv.data import images as I
    L = _lib.lib()
    frs = K.frames()
    f = frs["f0"]
    plain = I.sample_geometry(f.shape[1], f.shape[0], 64, 64, True, 0.5, 1, False)
    flagged = I.sample_geometry(f.shape[1], f.shape[0], 64, 64, True, 0.5, 1, False)
    flagged.fx = I.ImageFx(sharpen=0.3)
    counts = []
    for geoms in ([plain, plain], [plain, flagged]):
        torch.cuda.synchronize()
        L.profile_begin()
        out = I.transform_batch([f, f], geoms)
        torch.cuda.synchronize()
        names = []
        for i in range(L.profile_stop()):
            ms, buf = ctypes.c_float(), ctypes.create_string_buffer(256)
            L.profile_read(i, ctypes.byref(ms), buf, 256)
            names.append(buf.value.decode())
        counts.append(sum("imgfx" in n for n in names))
        assert len(names) == 2 + counts[-1], names
    assert counts == [0, 1]
    assert torch.equal(out[0], I.transform_batch([f], [plain])[0])                           # the unflagged image of a flagged batch: a copy
