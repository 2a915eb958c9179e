"""Mosaic augmentation on the device (csrc/mosaic.hip behind include/mdcv_aug.h, mdcv.data.MosaicBatches) against the NumPy
restatement tests/helpers/mosaic_ref.py: pixels as bytes, label rows as bits, the counters, all with `==`."""
import contextlib
import io
import itertools
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mosaic_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MINI = os.path.join(G, "mini")
SENTINEL = 0x7FC5A5A5                    # a NaN payload nothing computes


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def guarded(n, pad, dtype=torch.float32):
    """-> (the whole buffer, its middle n elements): `pad` sentinel words in front and behind"""
    whole = torch.full((pad + n + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    return whole, whole[pad:pad + n].view(dtype)


def sentinels_intact(whole, n, pad):
    w = whole.cpu().numpy()
    return bool((w[:pad] == SENTINEL).all() and (w[pad + n:] == SENTINEL).all())


def run(desc, imgs, tg, T_out, min_px=2.0, min_visible=0.25, desc_dev=None, pad=64, stats0=(0, 0, 0, 0)):
    """one call of the entry -> (out, targets_out, stats) as NumPy; `desc_dev`: another device copy than the host rows; the outputs lie
    between sentinel words, which must survive"""
    from mdcv import _lib
    A = _lib.aug_lib()
    desc = np.ascontiguousarray(desc, np.int32)
    B, C, H, W = imgs.shape
    T = tg.shape[1]
    d_desc = torch.from_numpy(desc if desc_dev is None else np.ascontiguousarray(desc_dev, np.int32)).cuda()
    d_in, d_tg = torch.from_numpy(imgs).cuda(), torch.from_numpy(tg).cuda()
    n_out, n_t = B * C * H * W, B * T_out * 5
    whole_o, out = guarded(n_out, pad)
    whole_t, tout = guarded(n_t, pad)
    stats = torch.tensor(stats0, dtype=torch.int32, device="cuda")
    A.check(A.mosaic_batch(desc.ctypes.data, d_desc.data_ptr(), B, C, H, W, d_in.data_ptr(), out.data_ptr(), d_tg.data_ptr(), T,
                           tout.data_ptr(), T_out, min_px, min_visible, stats.data_ptr(), torch.cuda.current_stream().cuda_stream),
            "mosaic_batch")
    torch.cuda.synchronize()
    assert sentinels_intact(whole_o, n_out, pad) and sentinels_intact(whole_t, n_t, pad)
    return out.cpu().numpy().reshape(B, C, H, W), tout.cpu().numpy().reshape(B, T_out, 5), stats.cpu().numpy()


def random_targets(g, B, T, full=False):
    tg = np.zeros((B, T, 5), np.float32)
    for b in range(B):
        n = T if full else int(g.integers(0, T + 1))
        tg[b, :n, 0] = g.integers(0, 3, n)
        tg[b, :n, 1:3] = g.uniform(0.02, 0.98, (n, 2))
        tg[b, :n, 3:5] = g.uniform(0.02, 0.5, (n, 2))
    return tg


# ---------------------------------------------------------------------------------------------------------------- pixels
@pytest.mark.parametrize("C", [3, 1])
def test_pixels_odd_width_every_centre(C):
    """W = 37: no row starts on a 16-byte boundary but every fourth, every row has cut cells at both ends; centres on the first and last
    column / row, at a multiple of 4 and off it.  Row 3 passes through, row 4 takes all four corners from one image.  Output buffers one
    word (pad 1) and 64 words behind a 16-byte boundary."""
    B, H, W = 5, 29, 37
    g = np.random.default_rng(11 + C)
    imgs = g.random((B, C, H, W), dtype=np.float32)
    imgs.view(np.uint32)[0, 0, :2, :5] = [0x7FC00001, 0xFFFFFFFF, 0x00000001, 0x80000000, 0x7F800000]      # copied as bits
    tg = random_targets(g, B, 3)
    for k, (xc, yc) in enumerate(itertools.product((1, 4, 18, 36), (1, 28))):
        desc = np.array([[1, xc, yc, *g.integers(0, B, 4), 0], [1, xc, H - yc, 4, 3, 2, 1, 0], [1, W - xc, yc, *g.integers(0, B, 4), 0],
                         [0, 0, 0, 0, 0, 0, 0, 0], [1, xc, yc, k % B, k % B, k % B, k % B, 0]], np.int32)
        want, want_t, want_s = R.mosaic(desc, imgs, tg, 12, 2.0, 0.25)
        for pad in (1, 64):
            out, tout, stats = run(desc, imgs, tg, 12, pad=pad)
            assert np.array_equal(u32(out), u32(want)), (xc, yc, pad, np.argwhere(u32(out) != u32(want))[:4])
            assert np.array_equal(u32(tout), u32(want_t)) and np.array_equal(stats, want_s)
        assert np.array_equal(u32(out[3]), u32(imgs[3])) and np.array_equal(u32(out[4, :, yc:, xc:]), u32(imgs[k % B, :, :H - yc, :W - xc]))


def test_pixels_at_the_network_size():
    """416 x 416: a row is two passes of a wave, the grid is several hundred blocks, W is a multiple of 4 (whole cells only)"""
    B, C, H, W = 4, 3, 416, 416
    g = np.random.default_rng(5)
    imgs = g.random((B, C, H, W), dtype=np.float32)
    tg = random_targets(g, B, 16)
    desc = np.array([[1, 105, 311, 3, 0, 1, 2, 0], [1, 208, 104, 1, 1, 0, 3, 0], [0, 0, 0, 0, 0, 0, 0, 0], [1, 415, 1, 2, 3, 0, 1, 0]], np.int32)
    want, want_t, want_s = R.mosaic(desc, imgs, tg, 64, 2.0, 0.25)
    out, tout, stats = run(desc, imgs, tg, 64)
    assert np.array_equal(u32(out), u32(want))
    assert np.array_equal(u32(tout), u32(want_t)) and np.array_equal(stats, want_s)


def test_pixels_beyond_the_grid_cap():
    """more rows than the capped grid's waves own in one pass (2048 blocks x 4 waves): the grid stride, at a tiny width"""
    B, C, H, W = 9, 4, 260, 6
    g = np.random.default_rng(8)
    imgs = g.random((B, C, H, W), dtype=np.float32)
    tg = random_targets(g, B, 2)
    desc = np.array([[int(b != 4), 1 + b % 5, 1 + 31 * b, *g.integers(0, B, 4), 0] for b in range(B)], np.int32)
    assert B * C * H > 2048 * 4
    want, want_t, want_s = R.mosaic(desc, imgs, tg, 8, 1.0, 0.0)
    out, tout, stats = run(desc, imgs, tg, 8, 1.0, 0.0)
    assert np.array_equal(u32(out), u32(want)) and np.array_equal(u32(tout), u32(want_t)) and np.array_equal(stats, want_s)


# ---------------------------------------------------------------------------------------------------------------- labels
def hand_labels():
    """W = 64, H = 48, centre (24, 20).  Quadrant 0 shows the source's x in [40, 64), y in [28, 48); quadrant 3 its x in [0, 40), y in [0, 28)."""
    nan, inf = np.float32("nan"), np.float32("inf")
    tg = np.array([
        [[1, 0.5, 0.5, 0.9, 0.9],            # straddles every cut: clipped into each quadrant
         [2, 0.0625, 0.0625, 0.0625, 0.125],  # the source's top-left corner: seen by quadrant 3 alone, hidden from the others
         [0, 0.125, 0.75, 0.25, 0.25]],       # left edge exactly on x = 0: in quadrant 1 / 3 it lands exactly on xc
        [[1, 0.875, 0.75, 0.25, 0.25],        # right edge exactly on x = W: in quadrant 0 / 2 it ends exactly on xc
         [0, nan, 0.5, 0.2, 0.2],             # a NaN: no candidate (its sum is not > 0), neither kept nor counted
         [2, inf, 0.5, 0.2, 0.2]],            # a candidate whose arithmetic meets inf - inf: dropped by the rule
        [[1, 0.6, 0.6, 0.5, 0.5],
         [0, 0, 0, 0, 0],                     # padded rows, one of them in front of a real row
         [2, 0.3, 0.3, 0.4, 0.4]],
        [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]],      # an image with no boxes
    ], np.float32)
    desc = np.array([[1, 24, 20, 0, 1, 2, 3, 0], [1, 24, 20, 1, 0, 0, 2, 0], [0, 0, 0, 0, 0, 0, 0, 0], [1, 24, 20, 3, 3, 3, 3, 0],
                     ], np.int32)
    return desc, tg


@pytest.mark.parametrize("T_out", [12, 5])
def test_labels_hand_made_rows(T_out):
    desc, tg = hand_labels()
    B, H, W = 4, 48, 64
    imgs = np.random.default_rng(1).random((B, 1, H, W), dtype=np.float32)
    want_t, want_s = R.labels(desc, tg, T_out, 2.0, 0.1, H, W)
    # the case holds what it is meant to: rows kept, rows dropped by the rule, and with T_out = 5 rows lost
    assert want_s[0] > 8 or T_out == 5
    assert want_s[1] >= 3 and (want_s[2] > 0) == (T_out == 5) and not want_t[3].any()
    assert any(want_t[1, i, 1] * 64 - want_t[1, i, 3] * 32 == 24 for i in range(T_out))          # a left edge exactly on xc
    _, tout, stats = run(desc, imgs, tg, T_out, 2.0, 0.1, stats0=(100, 200, 300, 0))
    assert np.array_equal(u32(tout), u32(want_t)), (tout, want_t)
    assert np.array_equal(stats, want_s + np.array([100, 200, 300, 0]))                         # accumulated, not reset


@pytest.mark.parametrize("T,T_out", [(300, 1200), (300, 333), (257, 256)])
def test_labels_longer_than_a_chunk(T, T_out):
    """T above the block size: the running count carries from chunk to chunk and from quadrant to quadrant; T_out cutting a chunk"""
    B = 3
    g = np.random.default_rng(T_out)
    tg = random_targets(g, B, T, full=True)
    tg[1, 100:180] = 0
    imgs = np.zeros((B, 1, 8, 8), np.float32)                    # an 8 x 8 canvas: boxes of up to 4 pixels, many of them cut away
    desc = np.array([[1, 3, 5, 2, 1, 0, 1, 0], [0, 0, 0, 0, 0, 0, 0, 0], [1, 7, 1, 0, 0, 2, 1, 0]], np.int32)
    want_t, want_s = R.labels(desc, tg, T_out, 1.0, 0.2, 8, 8)
    assert want_s[0] > 256 and want_s[1] > 0
    _, tout, stats = run(desc, imgs, tg, T_out, 1.0, 0.2)
    assert np.array_equal(u32(tout), u32(want_t)) and np.array_equal(stats, want_s)


# ---------------------------------------------------------------------------------------------------------------- corrupt device copy
def test_a_corrupt_device_descriptor_passes_the_image_through():
    B, C, H, W = 5, 3, 29, 37
    g = np.random.default_rng(21)
    imgs = g.random((B, C, H, W), dtype=np.float32)
    tg = random_targets(g, B, 3, full=True)
    desc = np.array([[1, 10 + b, 9 + b, *g.integers(0, B, 4), 0] for b in range(B)], np.int32)
    bad = desc.copy()
    bad[1, 1], bad[1, 4] = W + 7, B
    out, tout, stats = run(desc, imgs, tg, 12, desc_dev=bad, pad=1)              # (run() checks the sentinel words around both outputs)
    want, want_t, want_s = R.mosaic(bad, imgs, tg, 12, 2.0, 0.25)
    assert stats[3] & 1 and want_s[3] == 1
    assert np.array_equal(u32(out[1]), u32(imgs[1])) and np.array_equal(u32(tout[1, :3]), u32(tg[1])) and not tout[1, 3:].any()
    assert np.array_equal(u32(out), u32(want)) and np.array_equal(u32(tout), u32(want_t)) and np.array_equal(stats, want_s)


# ---------------------------------------------------------------------------------------------------------------- the wrapper
def test_mosaic_batches_over_a_list_of_device_batches():
    from mdcv import _lib
    from mdcv.data import MosaicBatches
    B, C, H, W, T = 4, 3, 29, 37, 3
    g = np.random.default_rng(31)
    host = [(g.random((B, C, H, W), dtype=np.float32), random_targets(g, B, T)) for _ in range(2)]
    batches = [([f"u{i}{b}" for b in range(B)], torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()) for i, (x, t) in enumerate(host)]
    rows = {(e, i): np.array([[int((b + i + e) % 3 != 0), 5 + 7 * i + b, 3 + 6 * e + b, *g.integers(0, B, 4), 0] for b in range(B)], np.int32)
            for e in (1, 2) for i in range(2)}
    m = MosaicBatches(batches, draws=lambda e, i, n: rows[(e, i)], min_px=2.0, min_visible=0.25)
    total = np.zeros(4, np.int64)
    for e in (1, 2):
        got = list(m)
        assert len(got) == 2 and m.epoch == e
        for i, (uris, out, tout) in enumerate(got):
            want, want_t, s = R.mosaic(rows[(e, i)], host[i][0], host[i][1], 4 * T, 2.0, 0.25)
            total += s
            assert uris is batches[i][0] and tuple(tout.shape) == (B, 4 * T, 5)
            assert np.array_equal(u32(out.cpu().numpy()), u32(want)) and np.array_equal(u32(tout.cpu().numpy()), u32(want_t))
            assert np.array_equal(u32(batches[i][1].cpu().numpy()), u32(host[i][0]))                    # the loader's batch is not written
    composed = int(sum(r[:, 0].sum() for r in rows.values()))
    assert m.stats() == dict(kept=int(total[0]), dropped=int(total[1]), overflow=0, errors=0, images=4 * B, composed=composed)
    assert m.summary_line("train", 2) == (f"train Epoch: 2, mosaic: {composed} of {4 * B} images composed, label rows kept {int(total[0])}, "
                                          f"dropped {int(total[1])}, overflow 0")
    m.active = False
    off = list(m)
    assert all(a is b for x, y in zip(off, batches) for a, b in zip(x, y)) and m.epoch == 2            # the very tensors of the loader
    assert "mosaic off" in m.summary_line("train", 3)
    # the default draws: a pure function of (seed, epoch, batch), the same batch from two wrappers
    a, b = [list(MosaicBatches(batches, p=0.7, seed=9)) for _ in range(2)]
    assert all(torch.equal(x[1].view(torch.int32), y[1].view(torch.int32)) and torch.equal(x[2].view(torch.int32), y[2].view(torch.int32))
               for x, y in zip(a, b))
    with pytest.raises(_lib.MdcvError, match="CPU tensor"):
        next(iter(MosaicBatches([(None, torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 5))])))


# ---------------------------------------------------------------------------------------------------------------- training
def mini_darknet():
    from mdcv.yolo.models import Darknet
    cwd = os.getcwd()
    os.chdir(MINI)
    try:
        net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32")
        net.load_weights("mini.weights", net.get_start_weight_dim())
    finally:
        os.chdir(cwd)
    return net.cuda().train()


def test_two_train_steps_on_mosaic_batches():
    from mdcv.data import MosaicBatches
    from mdcv.optim import FusedAdam
    from mdcv.yolo.train import run_epoch
    z = np.load(os.path.join(G, "mini_darknet.npz"))
    x, tg = torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["targets"]).cuda()
    loader = MosaicBatches([(["a", "b"], x, tg), (["c", "d"], x.flip(0).contiguous(), tg.flip(0).contiguous())], seed=3)
    net = mini_darknet()
    lines, stats = [], {}
    sums, _, count = run_epoch("train", loader, 100, FusedAdam(net, lr=1e-3), net, 1, 1, [0], log=lines.append, stats=stats)   # no IndexError
    assert stats == {"host_waits": 1, "steps": 2}
    assert len(sums) == 7 and all(np.isfinite(v) for v in sums) and sums[0] > 0 and count >= 1
    s = loader.stats()
    assert s["images"] == s["composed"] == 4 and s["kept"] >= 1 and s["overflow"] == 0
    assert abs(count - s["kept"]) < 1e-6                           # the model counted exactly the rows the mosaic kept


def test_train_wraps_the_training_loader_only_and_switches_it_off(tmp_path, monkeypatch):
    from mdcv.data import mosaic as mosaic_mod
    from mdcv.yolo import train as yt
    made = []

    class Recorded(mosaic_mod.MosaicBatches):
        def __init__(self, loader, **kw):
            made.append((loader, kw))
            super().__init__(loader, **kw)

    monkeypatch.setattr(mosaic_mod, "MosaicBatches", Recorded)
    os.makedirs(tmp_path / "dataset")
    for f in ("mini.cfg", "mini.weights"):
        shutil.copy(os.path.join(MINI, f), tmp_path / f)
    anchors = open(os.path.join(MINI, "dataset", "train.csv")).readline()
    rows = open(os.path.join(G, "imgload", "dataset.csv")).read().splitlines()[1:]
    for f in ("train.csv", "validate.csv"):
        with open(tmp_path / "dataset" / f, "w") as fh:
            fh.write(anchors.rstrip("\n") + "\n" + "\n".join(rows) + "\n")
    z = np.load(os.path.join(G, "imgload", "frames.npz"))
    frames = {k: z[k] for k in z.files}
    monkeypatch.chdir(tmp_path)
    os.makedirs("out")
    args = dict(evaluate=False, batch_size=2, optimizer_pick="Adam", model_cfg="mini.cfg", weights_path="mini.weights", output_path="out",
                dataset_path="", num_epochs=2, num_steps=1000, checkpoint_interval=2, augment_affine=False, augment_hsv=False, lr_flip=False,
                ud_flip=False, momentum=0.9, gamma=0.95, lr=1e-3, weight_decay=0.0, vis_batch=0, data_aug=False, blur=False, salt=False,
                noise=False, contrast=False, sharpen=False, ts=False, debug_mode=False, upload_dataset=False, xy_loss=2.0, wh_loss=1.6,
                no_object_loss=25.0, object_loss=0.1, vanilla_anchor=False, val_tolerance=3, min_epochs=0, num_workers=1)
    lines = []
    with contextlib.redirect_stdout(io.StringIO()):
        yt.train(**args, decode=lambda p: frames[os.path.splitext(os.path.basename(p))[0]], log=lines.append, mosaic=1.0, mosaic_off_epochs=1)
    assert len(made) == 1 and made[0][1] == {"p": 1.0} and made[0][0].shuffle                     # the training loader, once
    extra = [l for l in lines if "mosaic" in l]
    assert len(extra) == 2
    m = re.fullmatch(r"train Epoch: 1, mosaic: (\d+) of (\d+) images composed, label rows kept (\d+), dropped (\d+), overflow 0", extra[0])
    batches = sum(l.startswith("train Epoch: 1, Batch:") for l in lines)
    assert m and m.group(1) == m.group(2) and 2 * batches - 1 <= int(m.group(1)) <= 2 * batches and batches >= 2      # every image of every batch
    assert extra[1] == "train Epoch: 2, mosaic off: batches handed through"
    assert lines.index(extra[0]) == lines.index("Completed epoch:  1") - 1
    # off, the default: no wrapper, no line
    made.clear()
    off = []
    with contextlib.redirect_stdout(io.StringIO()):
        yt.train(**dict(args, num_epochs=1, checkpoint_interval=1), decode=lambda p: frames[os.path.splitext(os.path.basename(p))[0]],
                 log=off.append)
    assert made == [] and not any("mosaic" in l for l in off)
