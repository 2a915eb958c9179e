"""Real-image loader on the GPU (csrc/imgload.hip, mdcv/data/images.py) against Pillow 12.2 and the reference's label helpers.
Golden data only (tests/golden/imgload, written by tests/golden/make_golden_imgload.py)."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imgload")
NAMES = ["f0", "f1", "f2", "f3"]
pytestmark = pytest.mark.gpu


def _npz(name):
    return np.load(os.path.join(G, name))


def _frames():
    z = _npz("frames.npz")
    return {k: z[k] for k in z.files}


def _cases():
    z = _npz("cases.npz")
    out = []
    for i in range(int(z["n"])):
        fi, ts, patch, flip, bw, W, H = (int(v) for v in z[f"c{i}_params"])
        out.append(dict(name=NAMES[fi], ts=bool(ts), patch=patch, flip=bool(flip), W=W, H=H, scale=float(z[f"c{i}_scale"]),
                        u8=z[f"c{i}_u8"]))
    return out


def _geom(I, c, frames):
    f = frames[c["name"]]
    return I.sample_geometry(f.shape[1], f.shape[0], c["W"], c["H"], c["ts"], c["scale"], c["patch"], c["flip"] and c["name"] != "f3")


def _want(u8):
    """to_tensor: float32 u8 / 255 (correctly rounded division), NCHW"""
    return torch.from_numpy(np.moveaxis(u8, -1, 0).astype(np.float32) / np.float32(255))


def _check(got, u8, what):
    want = _want(u8)
    got = got.cpu()
    assert got.shape == want.shape, what
    back = torch.round(got * 255).to(torch.uint8).numpy()
    assert int((back != np.moveaxis(u8, -1, 0)).sum()) == 0, what              # 0 differing bytes before /255
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), what     # exact fp32 after it


def test_kernel_pair_matches_pillow_on_every_fixture():
    from mdcv.data import images as I
    frames = _frames()
    for c in _cases():
        g = _geom(I, c, frames)
        imgs = I.transform_batch([frames[c["name"]]], [g], bw=c["u8"].shape[2] == 1)
        _check(imgs[0], c["u8"], (c["name"], c["ts"], c["patch"], c["W"], c["H"]))


def test_mixed_size_batch_is_one_launch_pair():
    from mdcv import _lib
    from mdcv.data import images as I
    frames = _frames()
    cs = [c for c in _cases() if (c["W"], c["H"]) == (64, 64) and c["u8"].shape[2] == 3]
    assert len({c["name"] for c in cs}) >= 3 and len({c["ts"] for c in cs}) == 2
    geoms = [_geom(I, c, frames) for c in cs]
    L = _lib.lib()
    torch.cuda.synchronize()
    L.profile_begin()
    imgs = I.transform_batch([frames[c["name"]] for c in cs], geoms)
    torch.cuda.synchronize()
    n = L.profile_stop()
    names = []
    for i in range(n):
        ms, buf = ctypes.c_float(), ctypes.create_string_buffer(256)
        L.profile_read(i, ctypes.byref(ms), buf, 256)
        names.append(buf.value.decode())
    assert n == 2 and "imgload_hpass" in names[0] and "imgload_vpass" in names[1], names
    for b, c in enumerate(cs):
        _check(imgs[b], c["u8"], (b, c["name"]))


def test_bad_descriptors_are_rejected():
    from mdcv import _lib
    from mdcv.data import images as I
    frames = _frames()
    c = _cases()[0]
    g = _geom(I, c, frames)
    w = I.crop_window(frames[c["name"]], g)
    p = I.pack_layout([g], [w.nbytes], 0)
    host = np.zeros(p.nbytes, np.uint8)
    I.pack_batch(host, p, [g], [w])
    dev = torch.from_numpy(host).cuda()
    out = torch.empty(1, 3, 64, 64, device="cuda")
    ws = torch.empty(int(I._lib.lib().imgload_workspace_bytes(1, p.max_scr_w, p.max_scr_h)), dtype=torch.uint8, device="cuda")
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    desc = host[:I.DESC * 4].view(np.int32)
    base = dev.data_ptr()

    def run(d, C=3, mw=p.max_scr_w, mh=p.max_scr_h, src_bytes=p.src_bytes):
        h = np.ascontiguousarray(d, np.int32)
        return L.imgload_batch(h.ctypes.data, base + p.desc_off, 1, base + p.coef_off, p.n_coefs, base + p.pix_off, src_bytes, mw, mh, C,
                               64, 64, ws.data_ptr(), out.data_ptr(), st)
    assert run(desc) == 0
    torch.cuda.synchronize()
    _check(out[0], c["u8"], "valid")
    for field, value in ((0, p.src_bytes), (1, 10 ** 6), (3, 0), (4, -1), (5, p.n_coefs), (6, -4), (7, p.max_scr_w + 1),
                         (8, p.max_scr_h + 1), (10, 10 ** 6), (17, 2), (18, 1)):
        d = desc.copy()
        d[field] = value
        assert run(d) == -1, (field, value)
    assert run(desc, C=2) == -1
    assert run(desc, src_bytes=p.src_bytes - 1) == -1
    assert run(desc, mw=p.max_scr_w - 1) == -1
    torch.cuda.synchronize()


def _loader(I, name, prefetch, workers=4):
    z = _npz(name)
    frames = _frames()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return z, I.ImageLabelBatches(os.path.join(G, "dataset.csv"), "", int(z["W"]), int(z["H"]), ts=name == "loader_ts.npz",
                                      lr_flip=True, batch_size=int(z["B"]), shuffle=False, num_workers=workers, prefetch=prefetch,
                                      decode=lambda p: frames[os.path.splitext(os.path.basename(p))[0]],
                                      draws=lambda e, i: tuple(int(v) for v in z[f"e{e}_draws"][i]))


@pytest.mark.parametrize("name", ["loader_ts.npz", "loader_pad.npz"])
@pytest.mark.parametrize("prefetch", [True, False])
def test_loader_batches_equal_the_golden_batches(name, prefetch):
    from mdcv.data import images as I
    z, ld = _loader(I, name, prefetch)
    B, n = int(z["B"]), len(z["files"])
    sizes = []
    for e in range(3):                                       # three epochs through the same three staging buffers
        for bi, (uris, imgs, tg) in enumerate(ld):
            sl = slice(bi * B, min(n, (bi + 1) * B))
            sizes.append(imgs.shape[0])
            assert uris == [f for f in ld.img_files[sl]]
            assert imgs.is_cuda and tg.is_cuda and imgs.dtype == torch.float32 and tg.dtype == torch.float32
            for b in range(imgs.shape[0]):
                _check(imgs[b], z[f"e{e}_u8"][sl][b], (name, e, bi, b))
            want = torch.from_numpy(z[f"e{e}_targets"][sl])
            assert torch.equal(tg.cpu().view(torch.int32), want.view(torch.int32)), (name, e, bi)
    assert sizes[-1] == n % B and len(sizes) == 3 * len(ld)    # the short last batch
    ld.close()


def test_prefetch_does_not_overwrite_staging_under_a_copy():
    """the consumer holds every batch of three epochs, with a slow consumer stream in front of each; results equal the golden ones"""
    from mdcv.data import images as I
    z, ld = _loader(I, "loader_ts.npz", True, workers=8)
    held = []
    a = torch.randn(2048, 2048, device="cuda")
    for e in range(3):
        for uris, imgs, tg in ld:
            for _ in range(4):
                a = torch.tanh(a @ a)                      # keeps the device busy while the next batches are staged
            held.append((e, imgs, tg))
    torch.cuda.synchronize()
    B, n = int(z["B"]), len(z["files"])
    per = len(ld)
    for k, (e, imgs, tg) in enumerate(held):
        bi = k % per
        sl = slice(bi * B, min(n, (bi + 1) * B))
        for b in range(imgs.shape[0]):
            _check(imgs[b], z[f"e{e}_u8"][sl][b], (e, bi, b))
        assert torch.equal(tg.cpu(), torch.from_numpy(z[f"e{e}_targets"][sl]))
    ld.close()


def test_mini_darknet_step_fed_by_the_loader():
    from mdcv.data import images as I
    from mdcv.yolo.models import Darknet
    z, ld = _loader(I, "loader_ts.npz", True)
    uris, imgs, tg = next(iter(ld))
    ld.close()
    B = int(z["B"])
    x_ref = torch.from_numpy(np.moveaxis(z["e0_u8"][:B], -1, 1).astype(np.float32) / np.float32(255))
    t_ref = torch.from_numpy(z["e0_targets"][:B])
    assert torch.equal(imgs.cpu(), x_ref) and torch.equal(tg.cpu(), t_ref)
    mini = os.path.join(os.path.dirname(G), "mini")
    losses = []
    for x, t in ((imgs, tg), (x_ref.cuda(), t_ref.cuda())):
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
