"""GPU parity of the key-point crop loader (csrc/kptload.hip through mdcv.data.ConeCropBatches) with tests/helpers/kptload_numpy.py, which
composes the oracle's restatements of prep_image and prep_label: bit for bit, NaN positions included."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import kptload_numpy as N  # noqa: E402
from oracle import synth_oracle as SO  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ["top", "mid_L_top", "mid_R_top", "mid_L_bot", "mid_R_bot", "bot_L", "bot_R"]
# up-scale, non-integer down-scale, exact 2x, identity, a one-pixel-wide source: odd sizes, so every crop after the first starts unaligned
SHAPES_80 = ((13, 9), (131, 97), (160, 160), (80, 80), (40, 1))
SHAPES_48 = ((10, 300), (13, 9), (47, 49), (48, 48), (96, 96))


@functools.lru_cache(maxsize=None)
def case(shapes, size):
    """crops, labels and the numpy reference of one batch; computed once, shared, never modified"""
    crops = [N.make_crop(h, w, 100 * i + size) for i, (h, w) in enumerate(shapes)]
    labels = [N.make_label(h, w, 100 * i + size) for i, (h, w) in enumerate(shapes)]
    ref = N.batch(crops, labels, size)
    for a in crops + labels + list(ref):
        a.setflags(write=False)
    return crops, labels, ref


def loader(crops, labels, size, batch_size, **kw):
    from mdcv.data import ConeCropBatches
    names = [f"crop_{i}.png" for i in range(len(crops))]
    table = {os.path.join("mem", n): c for n, c in zip(names, crops)}
    return ConeCropBatches(names, labels, "mem", size, batch_size, decode=lambda p: table[p], **kw)


def check(batch, ref, sl=slice(None)):
    imgs, hm, pts = (t.cpu().numpy() for t in batch[:3])
    np.testing.assert_array_equal(imgs, ref[0][sl])
    np.testing.assert_array_equal(hm, ref[1][sl])                            # assert_array_equal wants NaNs at equal positions
    np.testing.assert_array_equal(pts, ref[2][sl])


def test_mixed_batch_bit_exact_at_80():
    crops, labels, ref = case(SHAPES_80, 80)
    ld = loader(crops, labels, 80, 5)
    assert len(ld) == 1 and len(ld.dataset) == 5
    (batch,) = list(ld)
    imgs, hm, pts, names, sizes = batch
    assert imgs.shape == (5, 3, 80, 80) and hm.shape == (5, 7, 80, 80) and pts.shape == (5, 7, 2)
    assert imgs.is_cuda and hm.is_cuda and pts.is_cuda and imgs.dtype == hm.dtype == pts.dtype == torch.float32
    check(batch, ref)
    assert names == [f"crop_{i}" for i in range(5)]
    assert len(sizes) == 3 and all(s.dtype == torch.int64 and s.shape == (5,) for s in sizes)
    assert sizes[0].tolist() == [h for h, _ in SHAPES_80] and sizes[1].tolist() == [w for _, w in SHAPES_80] and sizes[2].tolist() == [3] * 5
    assert np.isfinite(ref[1]).all() and ld.incorrect_labels == []
    ld.close()


@pytest.mark.parametrize("size", [48, 50, 16, 256])                            # 50: no 16-byte stores; 16 and 256: the bounds of the LDS tables
def test_other_sizes_bit_exact(size):
    shapes = SHAPES_48 if size == 48 else SHAPES_48[:2]
    crops, labels, ref = case(shapes, size)
    from mdcv.data import crops as C
    check(C.transform_batch(crops, labels, size), ref)
    if size == 48:
        (batch,) = list(loader(crops, labels, size, len(crops)))
        check(batch, ref)


def test_channel_order_is_bgr():
    from mdcv.data import crops as C
    crop = np.empty((21, 33, 3), np.uint8)
    crop[:] = (10, 20, 30)                                                   # R, G, B planes: three different constants
    imgs, _, _ = C.transform_batch([crop], [np.full((7, 2), 4.0)], 80)
    for plane, v in enumerate((30, 20, 10)):
        assert (imgs[0, plane].cpu().numpy() == np.float32(v / 255.0)).all()


def test_corner_hot_pixels():
    from mdcv.data import crops as C
    shapes = ((30, 20), (80, 80), (131, 97), (24, 71))
    crops = [N.make_crop(h, w, 5 + i) for i, (h, w) in enumerate(shapes)]
    labels = []
    for h, w in shapes:
        lab = N.make_label(h, w, h)
        lab[0] = (0.0, 0.0)
        lab[1] = (w - 1, h - 1)
        lab[2] = (w - 0.01, 0.3)                                             # int() -> (w - 1, 0)
        labels.append(lab)
    imgs, hm, pts = C.transform_batch(crops, labels, 80)
    check((imgs, hm, pts), N.batch(crops, labels, 80))
    s = hm.double().sum((2, 3)).cpu().numpy()
    np.testing.assert_allclose(s, 1.0, atol=1e-5)
    peak = hm.flatten(2).argmax(2).cpu().numpy()
    p = pts.cpu().numpy() * 80
    assert np.all(np.abs(peak % 80 - p[..., 0]) <= 4) and np.all(np.abs(peak // 80 - p[..., 1]) <= 4)


def test_missed_tap_gives_the_reference_nan_map(capsys):
    h, w = 40, 200
    crops = [N.make_crop(h, w, 1), N.make_crop(50, 60, 2)]
    labels = [N.make_label(h, w, 1), N.make_label(50, 60, 2)]
    labels[0][:, 0] = (3.2, 20.5, 2.7, 50.1, 100.9, 150.0, 199.0)            # 200 -> 80 never reads source column 2
    ld = loader(crops, labels, 80, 2)
    (batch,) = list(ld)
    check(batch, N.batch(crops, labels, 80))
    hm = batch[1].cpu().numpy()
    assert np.isnan(hm[0, 2]).all()
    assert np.isfinite(hm[0, [0, 1, 3, 4, 5, 6]]).all() and np.isfinite(hm[1]).all()
    assert ld.incorrect_labels == ["crop_0.png"]
    out = capsys.readouterr().out
    assert "Incorrect Data Label Detected!" in out and "crop_0.png" in out


def test_batch_of_one_and_short_last_batch():
    shapes = SHAPES_80 + ((57, 33), (24, 90))
    crops, labels, ref = case(shapes, 80)
    ld = loader(crops, labels, 80, 3)
    assert len(ld) == 3 and len(ld.dataset) == 7
    got = list(ld)
    assert [b[0].shape[0] for b in got] == [3, 3, 1]
    for i, b in enumerate(got):
        check(b, ref, slice(3 * i, 3 * i + 3))
        assert b[3] == [f"crop_{j}" for j in range(3 * i, min(7, 3 * i + 3))]
    assert got[2][4][0].tolist() == [24] and got[2][4][1].tolist() == [90]
    val = list(loader(crops, labels, 80, 1))                                 # the validation loader's batch
    assert len(val) == 7
    for i, b in enumerate(val):
        check(b, ref, slice(i, i + 1))


def test_prefetch_on_and_off_agree():
    crops, labels, ref = case(SHAPES_80 + ((57, 33), (24, 90)), 80)
    a = list(loader(crops, labels, 80, 2, prefetch=True))
    b = list(loader(crops, labels, 80, 2, prefetch=False, num_workers=1))
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        for t, u in zip(x[:3], y[:3]):
            assert torch.equal(t.view(torch.int32), u.view(torch.int32))      # bit patterns
        assert x[3] == y[3] and all(torch.equal(s, t) for s, t in zip(x[4], y[4]))
    for i, x in enumerate(a):
        check(x, ref, slice(2 * i, 2 * i + 2))


def test_bounds_return_earg_and_launch_nothing():
    from mdcv import _lib
    from mdcv.data import crops as C
    L = _lib.lib()
    side = C.MAX_SIDE + 1
    host = np.zeros((1, C.DESC), np.int32)
    dev = torch.zeros(C.DESC, dtype=torch.int32, device="cuda")
    src = torch.zeros(3 * side, dtype=torch.uint8, device="cuda")
    imgs = torch.full((1, 3, 264, 264), 7.0, device="cuda")
    hm = torch.full((1, 7, 264, 264), 7.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(h, w, size, hot=(0, 0), nbytes=None):
        host[0, :] = 0
        host[0, 1:3] = h, w
        host[0, 4:18] = list(hot) * 7
        dev.copy_(torch.from_numpy(host[0]))
        return L.kptload_batch(host.ctypes.data, dev.data_ptr(), 1, src.data_ptr(), src.numel() if nbytes is None else nbytes, size,
                               imgs.data_ptr(), hm.data_ptr(), st)

    assert call(8, 8, 8) == -1 and call(8, 8, 264) == -1 and call(8, 8, 15) == -1 and call(8, 8, 257) == -1
    assert call(side, 1, 80) == -1 and call(1, side, 80) == -1 and call(0, 5, 80) == -1 and call(5, 0, 80) == -1
    assert call(8, 8, 80, nbytes=8 * 8 * 3 - 1) == -1                        # the crop ends past src
    assert call(8, 8, 80, hot=(8, 0)) == -1 and call(8, 8, 80, hot=(0, 8)) == -1 and call(8, 8, 80, hot=(-1, 0)) == -1
    torch.cuda.synchronize()
    assert bool((imgs == 7.0).all()) and bool((hm == 7.0).all())             # nothing was enqueued
    assert call(8, 8, 16) == 0 and call(C.MAX_SIDE, 1, 256) == 0 and call(1, C.MAX_SIDE, 256) == 0     # the bounds themselves are accepted
    torch.cuda.synchronize()
    assert bool((imgs.flatten()[:3 * 256 * 256] == 0.0).all())


def test_training_step_from_files(tmp_path, capsys):
    """PNG crops + CSV -> load_train_csv_dataset -> ConeCropBatches -> KeypointNet + CrossRatioLoss + FusedAdam: 8 steps on one batch"""
    from PIL import Image
    from mdcv.data import ConeCropBatches, load_train_csv_dataset
    from mdcv.optim import FusedAdam
    from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss
    from mdcv.rektnet.keypoint_net import KeypointNet
    rng = np.random.default_rng(0)
    rows = ["image,url," + ",".join(KEYS)]
    for i in range(32):
        h, w = int(rng.integers(24, 161)), int(rng.integers(24, 161))
        Image.fromarray(N.make_crop(h, w, i)).save(tmp_path / f"cone_{i}.png")
        kp = np.clip(SO.KP.astype(np.float64) + rng.uniform(-0.02, 0.02, (7, 2)), 0, 0.999) * (w, h)
        rows.append(",".join([f"cone_{i}.png", "u"] + [f'"({x:.2f},{y:.2f})"' for x, y in kp]))
    (tmp_path / "labels.csv").write_text("\n".join(rows) + "\n")
    ti, tl, vi, vl = load_train_csv_dataset(str(tmp_path / "labels.csv"), 0.0, KEYS, str(tmp_path) + "/")
    assert len(ti) == 32 and len(vi) == 0
    ld = ConeCropBatches(ti, tl, str(tmp_path) + "/", (80, 80), 32)
    (batch,) = list(ld)
    ld.close()
    imgs, hm_t, pts_t, names, sizes = batch
    assert imgs.shape == (32, 3, 80, 80) and names[0] == "cone_0" and bool(torch.isfinite(hm_t).all())
    torch.manual_seed(0)
    kp = KeypointNet(7, (80, 80), precision="bf16").cuda().train()
    crit = CrossRatioLoss("l1_softargmax", True, 0.05, 0.05)
    opt = FusedAdam(kp, lr=1e-2)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        hm, pts = kp(imgs)
        loss = crit(hm, pts, hm_t, pts_t)[2]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
