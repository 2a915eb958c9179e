"""Key-point augmentation on the device (csrc/kptaug.hip behind include/mdcv_kptaug.h, mdcv.data.KeypointAugBatches) against the
NumPy restatement tests/kptaug_ref.py: pixels, heat-maps and points as bit patterns, the counters, all with `==`; and against anchors that
need no restatement (the identity, quarter turns, a mirror)."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import kptaug_ref as R
from oracle.synth_oracle import cone_crops

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0x7FC5A5A5                    # a NaN payload nothing computes


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(u32(a), u32(b))


def guarded(n, pad):
    """-> (the whole buffer, its middle n elements as float32): `pad` sentinel words in front and behind"""
    whole = torch.full((pad + n + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    return whole, whole[pad:pad + n].view(torch.float32)


def intact(whole, n, pad):
    w = whole.cpu().numpy()
    return bool((w[:pad] == SENTINEL).all() and (w[pad + n:] == SENTINEL).all())


def run(desc, imgs, hm, pts, desc_dev=None, pad=64, stats0=(0, 0, 0, 0)):
    """one call of the entry -> (imgs_out, hm_out, pts_out, stats) as NumPy; `desc_dev`: another device copy than the host rows; the
    outputs lie between sentinel words, which must survive.  pad = 1 puts every output one word behind a 16-byte boundary."""
    from mdcv import _lib
    A = _lib.kptaug_lib()
    desc = np.ascontiguousarray(desc, np.int32).reshape(-1, 24)
    B, C, S, _ = imgs.shape
    d_desc = torch.from_numpy(desc if desc_dev is None else np.ascontiguousarray(desc_dev, np.int32)).cuda()
    d_in = [torch.from_numpy(np.array(a)).cuda() for a in (imgs, hm, pts)]
    sizes = [B * C * S * S, B * 7 * S * S, B * 14]
    outs = [guarded(n, pad) for n in sizes]
    stats = torch.tensor(stats0, dtype=torch.int32, device="cuda")
    A.check(A.kptaug_batch(desc.ctypes.data, d_desc.data_ptr(), B, C, S, 7, *[t.data_ptr() for t in d_in], *[o[1].data_ptr() for o in outs],
                           stats.data_ptr(), torch.cuda.current_stream().cuda_stream), "kptaug_batch")
    torch.cuda.synchronize()
    assert all(intact(o[0], n, pad) for o, n in zip(outs, sizes))
    assert all(same(t.cpu().numpy(), a) for t, a in zip(d_in, (imgs, hm, pts)))          # the inputs are not written
    return (outs[0][1].cpu().numpy().reshape(B, C, S, S), outs[1][1].cpu().numpy().reshape(B, 7, S, S),
            outs[2][1].cpu().numpy().reshape(B, 7, 2), stats.cpu().numpy())


@functools.lru_cache(maxsize=None)
def crops(S, B, C=3, seed=5):
    """random pixels in [0, 1], heat-maps and points of the synthetic crop oracle at size S (computed once per shape, never written)"""
    _, hm, pts = cone_crops(seed, S, B, size=S)
    imgs = np.random.default_rng(S * 131 + B * 7 + C).random((B, C, S, S), dtype=F)
    for a in (imgs, hm, pts):
        a.setflags(write=False)
    return imgs, hm, pts


def check(desc, imgs, hm, pts, **kw):
    want = R.kptaug(kw.get("desc_dev", desc), imgs, hm, pts)                     # the kernel reads the device copy
    got = run(desc, imgs, hm, pts, **kw)
    for name, g, w in zip(("imgs", "hm", "pts"), got, want):
        assert same(g, w), (name, np.argwhere(u32(g) != u32(w))[:4])
    assert np.array_equal(got[3], want[3] + np.array(kw.get("stats0", (0, 0, 0, 0)), np.int32)), (got[3], want[3])          # accumulated
    return got


SHAPES = [(16, 1, 3), (18, 3, 3), (80, 5, 3), (256, 2, 3), (80, 5, 1), (18, 3, 1)]


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("S,B,C", SHAPES)
def test_drawn_rows_against_the_restatement(S, B, C):
    """the wrapper's own draws, shrinking so that the synthetic cones' border-hugging points stay inside; pad 1 takes the scalar stores at
    every S"""
    from mdcv.data.kptaug import draw_rows
    imgs, hm, pts = crops(S, B, C)
    desc = draw_rows(S, 1, 0, B, S, degrees=8.0, scale=(0.7, 0.85), translate=0.01)
    got = check(desc, imgs, hm, pts)
    assert got[3][0] >= 1 and got[3][3] == 0 and got[3][:3].sum() == B
    assert np.isfinite(got[1]).all() and got[0].min() >= 0.0 and got[0].max() <= 1.0
    if S < 256:
        check(desc, imgs, hm, pts, pad=1)


def test_wild_rows_never_leave_the_buffers():
    """maps that send every pixel far outside (huge, tiny, overflowing to inf - inf): the clamps hold, the sentinels survive (run())"""
    S, B = 18, 4
    imgs, hm, pts = crops(S, B)
    ident = (1, 0, 0, 0, 1, 0)
    desc = [R.row(I=(3e38, 3e38, -3e38, -3e38, 3e38, 3e38), Fw=ident), R.row(I=(1e-30, 0, -1e9, 0, 1e-30, 1e9), Fw=ident),
            R.row(I=(-7.5, 2.25, 40, 3.5, -9, 300), Fw=ident), R.row(I=ident, Fw=(3e38, 3e38, -3e38, 0, 1, 0))]
    got = check(desc, imgs, hm, pts, pad=1)
    assert got[3].tolist() == [3, 1, 0, 0]                                         # the last row's points are inf - inf: NaN, rejected


# ---------------------------------------------------------------------------------------------------------------- anchors
@pytest.mark.parametrize("S,C", [(16, 3), (18, 1), (80, 3)])
def test_identity_and_quarter_turns_without_the_restatement(S, C):
    imgs, hm, _ = crops(S, 4, C)
    pts = np.full((4, 7, 2), 0.5, F)                                               # the centre stays inside under every turn
    n = S - 1
    I = [(1, 0, 0, 0, 1, 0), (0, -1, n, 1, 0, 0), (-1, 0, n, 0, -1, n), (0, 1, 0, -1, 0, n)]       # np.rot90(m, k): out[y, x] = m[sy, sx]
    Fw = [(1, 0, 0, 0, 1, 0), (0, 1, 0, -1, 0, n), (-1, 0, n, 0, -1, n), (0, -1, n, 1, 0, 0)]      # their inverses
    oi, oh, op, stats = run([R.row(I=i, Fw=f) for i, f in zip(I, Fw)], imgs, hm, pts)
    assert stats.tolist() == [4, 0, 0, 0]
    for k in range(4):
        assert same(oi[k], np.rot90(imgs[k], k, axes=(1, 2))), k
    h = F(S / 2)
    want = [(h, h), (h, F(n) - h), (F(n) - h, F(n) - h), (F(n) - h, h)]
    for k in range(4):
        assert (op[k, :, 0] == want[k][0] / F(S)).all() and (op[k, :, 1] == want[k][1] / F(S)).all()
        y, x = np.unravel_index(np.argmax(oh[k, 0]), (S, S))
        assert (x, y) == (int(want[k][0]), int(want[k][1])) and abs(float(oh[k].sum()) - 7.0) < 1e-4


@pytest.mark.parametrize("S", [16, 18])
def test_a_mirror_without_the_restatement(S):
    from mdcv.data.kptaug import descriptor
    imgs, hm, pts = crops(S, 3)
    pts = np.minimum(pts, F((S - 2) / S))                                          # a point beyond S - 1 would mirror below 0: keep all inside
    oi, oh, op, stats = run([descriptor(S, flip=True)] * 3, imgs, hm, pts)
    assert stats.tolist() == [3, 0, 0, 0]
    assert same(oi, imgs[..., ::-1])
    want = pts[:, list(R.PERM)].copy()
    want[..., 0] = (F(S - 1) - want[..., 0] * F(S)) / F(S)
    want[..., 1] = (want[..., 1] * F(S)) / F(S)
    assert same(op, want)
    assert not same(oh, hm) and np.isfinite(oh).all()


def test_the_colour_clamp_at_both_ends():
    S = 16
    imgs, hm, _ = crops(S, 2)
    pts = np.full((2, 7, 2), 0.5, F)
    desc = [R.row(gain=(4, -1, 1), bias=(-1.5, 0.5, 0.25)), R.row(gain=(0, 0, 0), bias=(-1, 2, 0.5))]
    oi, _, _, _ = check(desc, imgs, hm, pts)
    want0 = np.clip(np.stack([imgs[0, 0] * F(4) + F(-1.5), imgs[0, 1] * F(-1) + F(0.5), imgs[0, 2] * F(1) + F(0.25)]), F(0), F(1))
    assert same(oi[0], want0) and (oi[0] == 0).any() and (oi[0] == 1).any() and ((oi[0] > 0) & (oi[0] < 1)).any()
    assert (oi[1, 0] == 0).all() and (oi[1, 1] == 1).all() and (oi[1, 2] == 0.5).all()


# ---------------------------------------------------------------------------------------------------------------- mixed rows
def mixed_case(S=18):
    imgs, hm, pts = (a.copy() for a in crops(S, 5))
    hm[0, 2, 3, 4] = np.nan                                                        # row 0 is not applied: the NaN passes as bits
    hm.view(np.uint32)[0, 0, 0, :2] = [0x7FC00001, 0x80000000]
    pts[2, 4] = [1.0, 1.0]                                                         # exactly 1.0: kept under the identity
    pts[3] = np.clip(pts[3], F(2 / S), F((S - 2) / S))                             # row 3 shifts by a fraction of a pixel: keep it inside
    push = float(S) - float(pts[1, :, 0].max()) * S + 0.5                          # row 1: a shift that takes its right-most point past Sf
    desc = np.stack([R.row(apply=0, swap=1, gain=(0, 0, 0)), R.row(I=(1, 0, -push, 0, 1, 0), Fw=(1, 0, push, 0, 1, 0)), R.row(),
                     R.row(I=(1, 0, 0.5, 0, 1, -0.25), Fw=(1, 0, -0.5, 0, 1, 0.25)), R.row(swap=1)])
    return desc, imgs, hm, pts


def test_mixed_rows_pass_through_reject_keep_and_report():
    desc, imgs, hm, pts = mixed_case()
    oi, oh, op, stats = check(desc, imgs, hm, pts, stats0=(100, 200, 300, 0))
    assert stats.tolist() == [103, 201, 301, 0]                                    # accumulated, not reset
    for b in (0, 1):
        assert same(oi[b], imgs[b]) and same(oh[b], hm[b]) and same(op[b], pts[b])
    assert same(oi[2], imgs[2]) and op[2, 4].tolist() == [1.0, 1.0] and np.isfinite(oh[2]).all()
    y, x = np.unravel_index(np.argmax(oh[2, 4]), oh[2, 4].shape)
    assert (x, y) == (17, 17)
    # a device copy whose row 3 went bad: that image passes through, counts as passed, and raises bit 0
    bad = desc.copy()
    bad[3, 0] |= 16
    oi, oh, op, stats = check(desc, imgs, hm, pts, desc_dev=bad, pad=1)
    assert stats.tolist() == [2, 1, 2, 1]
    assert same(oi[3], imgs[3]) and same(oh[3], hm[3]) and same(op[3], pts[3])
    bad = desc.copy()
    bad[4, 9] = 0x7FC00000                                                         # a NaN in F
    bad[2, 21] = 5                                                                 # a pad word
    assert check(desc, imgs, hm, pts, desc_dev=bad)[3].tolist() == [1, 1, 3, 1]


# ---------------------------------------------------------------------------------------------------------------- the wrapper
def device_batches(S=80, B=3, n=2):
    host = [crops(S, B, 3, seed=20 + i) for i in range(n)]
    return host, [(*[torch.from_numpy(a.copy()).cuda() for a in h], [f"c{i}_{b}" for b in range(B)], [(S, S, 3)] * B) for i, h in enumerate(host)]


def test_the_wrapper_over_three_epochs_of_two_batches():
    from mdcv import _lib
    from mdcv.data import KeypointAugBatches
    from mdcv.data.kptaug import draw_rows
    host, batches = device_batches()
    m = KeypointAugBatches(batches, p=0.8, seed=4)
    total = np.zeros(4, np.int64)
    for e in (1, 2, 3):
        got = list(m)
        assert len(got) == 2 and m.epoch == e
        for i, (oi, oh, op, names, sizes) in enumerate(got):
            want = R.kptaug(draw_rows(4, e, i, 3, 80, p=0.8), *host[i])
            total += want[3]
            assert names is batches[i][3] and sizes is batches[i][4]
            assert same(oi.cpu().numpy(), want[0]) and same(oh.cpu().numpy(), want[1]) and same(op.cpu().numpy(), want[2])
            assert all(same(batches[i][j].cpu().numpy(), host[i][j]) for j in range(3))          # the loader's batch is not written
    assert total[0] >= 1 and total[1] >= 1 and total[3] == 0                       # (the defaults reject the draws that push a border point out)
    assert m.stats() == dict(augmented=int(total[0]), rejected=int(total[1]), passed=int(total[2]), errors=0, images=18)
    assert m.summary_line("train", 3) == (f"train Epoch: 3, key-point augmentation: {int(total[0])} of 18 images augmented, "
                                          f"rejected {int(total[1])}, passed through {int(total[2])}")
    # the same (seed, epoch, index) gives the same bits, from another wrapper
    a, b = [list(KeypointAugBatches(batches, seed=9)) for _ in range(2)]
    assert all(torch.equal(x[j].view(torch.int32), y[j].view(torch.int32)) for x, y in zip(a, b) for j in range(3))
    c = list(KeypointAugBatches(batches, seed=10))
    assert not all(torch.equal(x[0], y[0]) for x, y in zip(a, c))
    # switched off: the very tensors of the loader, no epoch of draws consumed
    m.active = False
    off = list(m)
    assert all(p is q for x, y in zip(off, batches) for p, q in zip(x, y)) and m.epoch == 3
    assert "augmentation off" in m.summary_line("train", 4)
    with pytest.raises(_lib.MdcvError, match="CPU tensor"):
        next(iter(KeypointAugBatches([(torch.zeros(1, 3, 16, 16), torch.zeros(1, 7, 16, 16), torch.zeros(1, 7, 2), ["a"], [(16, 16, 3)])])))


def test_stats_raises_on_a_device_side_bad_row():
    from mdcv import _lib
    from mdcv.data import KeypointAugBatches
    desc, imgs, hm, pts = mixed_case()
    t = [torch.from_numpy(a).cuda() for a in (imgs, hm, pts)]
    m = KeypointAugBatches([], draws=lambda e, i, B: desc)
    out = m.augment(m.rows(1, 0, 5, 18), *t)
    assert m.stats() == dict(augmented=3, rejected=1, passed=1, errors=0, images=5)
    bad = desc.copy()
    bad[3, 0] |= 16
    A = _lib.kptaug_lib()
    A.check(A.kptaug_batch(desc.ctypes.data, torch.from_numpy(bad).cuda().data_ptr(), 5, 3, 18, 7, *[x.data_ptr() for x in t],
                           *[x.data_ptr() for x in out], m._stats.data_ptr(), torch.cuda.current_stream().cuda_stream), "kptaug_batch")
    with pytest.raises(_lib.MdcvError, match="rejected a device descriptor"):
        m.stats()
    assert same(out[0][3].cpu().numpy(), imgs[3])


# ---------------------------------------------------------------------------------------------------------------- training
def test_train_model_with_augment_adds_one_line_and_no_wait(monkeypatch):
    from mdcv.data import SyntheticConeCrops
    from mdcv.data import kptaug as KA
    from mdcv.optim import FusedAdam
    from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss
    from mdcv.rektnet.keypoint_net import KeypointNet
    from mdcv.rektnet.train import train_model
    made = []

    class Recorded(KA.KeypointAugBatches):
        def __init__(self, loader, **kw):
            made.append((loader, kw))
            super().__init__(loader, **kw)

    monkeypatch.setattr(KA, "KeypointAugBatches", Recorded)
    val = [tuple(t.clone() if torch.is_tensor(t) else t for t in b) for b in SyntheticConeCrops(4, batches=1, seed=8)]
    val_before = [[t.clone() for t in b[:3]] for b in val]

    def once(**kw):
        torch.manual_seed(0)
        model = KeypointNet(7, (80, 80)).cuda()
        with contextlib.redirect_stdout(io.StringIO()):
            loss_function = CrossRatioLoss("l1_softargmax", False, 0.05, 0.05)
            optimizer = FusedAdam(model, lr=1e-3)
            scheduler = torch.optim.lr_scheduler.ExponentialLR(optimizer, gamma=0.9)
            lines, stats = [], {}
            loader = kw.pop("loader", None) or SyntheticConeCrops(4, batches=2, seed=7)
            train_model(model, "unused", loader, loss_function, optimizer, scheduler, 2, val, 10, (80, 80), 7, False,
                        ["k%d" % k for k in range(7)], "study", False, log=lines.append, stats=stats, **kw)
        return lines, stats

    plain, plain_stats = once()
    assert made == [] and not any("augmentation" in l for l in plain)
    lines, stats = once(augment=dict(seed=3, degrees=5.0))
    assert len(made) == 1 and made[0][1] == dict(seed=3, degrees=5.0) and isinstance(made[0][0], SyntheticConeCrops)      # the training loader, once
    assert stats["host_waits"] == plain_stats["host_waits"] and len(stats["host_waits"]) == 2
    extra = [l for l in lines if "key-point augmentation" in l]
    assert len(lines) == len(plain) + 2 and len(extra) == 2
    for e, l in enumerate(extra):
        assert l.startswith(f"train Epoch: {e}, key-point augmentation: ") and " of 8 images augmented, rejected " in l
        assert lines[lines.index(l) - 1].startswith("\tTraining:")
    rest = [l for l in lines if l not in extra]
    assert [l.split(":")[0] for l in rest] == [l.split(":")[0] for l in plain]                   # the other lines: the same kinds, in order
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for x, y in zip(val, val_before) for a, b in zip(x[:3], y))
    # a loader that already is a wrapper is used as it is
    own = KA.KeypointAugBatches(SyntheticConeCrops(4, batches=2, seed=7), seed=3, degrees=5.0)
    made.clear()
    again, _ = once(loader=own)
    assert made == [] and own.epoch == 2 and [l for l in again if "key-point augmentation" in l] == extra
