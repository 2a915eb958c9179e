"""-m gpu: the opt-in prediction-IoU ignore rule of the YOLO head's no-object term (csrc/yolo_ign.hip, include/mdcv_ign.h) against a float64
torch-CPU restatement on the logits as the dtype stores them.  The decision is a threshold, so every case first asserts on the reference
alone that no unowned cell's best IoU lies within 1e-4 of thr (fp32 expf at a few ulp and about ten operations: 1e-6 relative on inter
and union, a band 100 times that) and, where the case is not degenerate, that 5-60 % of the negatives are ignored.  Then the mask, n and
nN' are compared with ==, values under test_gpu_heads.py's rule unchanged (`compare`), every other byte with the head alone."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mdcv import _lib  # noqa: E402
from test_gpu_heads import F32, BF16, ITYPE, P, YoloCase, compare, head_counts, hr, rnd, run_train, st, sync  # noqa: E402
from test_gpu_yolo_cls import step  # noqa: E402

F64, BAND, NOOBJ = torch.float64, 1e-4, 25.0
DT = pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])


def label_boxes(case, targets):
    """real rows [B,T] (the head's fp32 sum, in its order) and the boxes of all rows in grid units [B,T,4] (the head's fp32 products)"""
    s = targets[..., 0]
    for k in range(1, 5):
        s = s + targets[..., k]
    return s > 0, targets[..., 1:] * torch.tensor([case.Gw, case.Gh, case.Gw, case.Gh], dtype=torch.float32)


def ious(case, targets):
    """float64 IoU of every cell's predicted box with every row of its image [B,3,Gh,Gw,T]; -1 for a padding row"""
    real, g = label_boxes(case, targets)
    z = case.sample.double().view(case.B, 3, case.attrs, case.Gh, case.Gw)
    an = hr.scaled_anchors(case.anchors_px, case.stride).double()
    jj, ii = torch.meshgrid(torch.arange(case.Gh), torch.arange(case.Gw), indexing="ij")
    px, py = torch.sigmoid(z[:, :, 0]) + ii, torch.sigmoid(z[:, :, 1]) + jj
    pw, ph = torch.exp(z[:, :, 2].clamp(max=20)) * an[:, 0, None, None], torch.exp(z[:, :, 3].clamp(max=20)) * an[:, 1, None, None]
    px, py, pw, ph = (t[..., None] for t in (px, py, pw, ph))
    gx, gy, gw, gh = (g[:, None, None, None, :, k].double() for k in range(4))
    iw = (torch.min(px + pw / 2, gx + gw / 2) - torch.max(px - pw / 2, gx - gw / 2)).clamp(min=0)
    ih = (torch.min(py + ph / 2, gy + gh / 2) - torch.max(py - ph / 2, gy - gh / 2)).clamp(min=0)
    iou = iw * ih / (pw * ph + gw * gh - iw * ih + 1e-7)
    return torch.where(real[:, None, None, None, :], iou, torch.full_like(iou, -1.0))


def ign_ref(case, thr, degenerate):
    """-> ignored cells, per-row IoU, owned cells, negatives (bool [B,3,Gh,Gw]); asserts the two preconditions on the reference alone"""
    iou = ious(case, case.targets)
    best = iou.max(-1).values
    pos, neg = case.masks()
    assert not bool((((best - thr).abs() <= BAND) & ~pos).any()), "an unowned cell's best IoU lies within 1e-4 of thr"
    ign = neg & (best > thr)
    assert degenerate or 0.05 <= int(ign.sum()) / int(neg.sum()) <= 0.60, (int(ign.sum()), int(neg.sum()))
    return ign, iou, pos, neg


def noobj_ref(case, keep, dtype):
    """-> loss_noobj over the cells `keep` and d loss_noobj / d conf logit of one of them (25 p / nN'), float64 tensors of `dtype` values"""
    p = hr.stable_sigmoid(case.sample.to(dtype).view(case.B, 3, case.attrs, case.Gh, case.Gw)[:, :, 4])
    bce = -torch.log(1 - p).clamp(min=-100)
    return (NOOBJ * bce[keep].sum() / keep.sum()).double(), (NOOBJ * p / keep.sum()).double()


def predict(case, b, j, i, box, gen):
    """all anchors of cell (b, j, i) predict `box`: the centre as near as the cell allows, the size jittered by -20 .. +25 % per anchor"""
    an, s = hr.scaled_anchors(case.anchors_px, case.stride), case.sample.view(case.B, 3, case.attrs, case.Gh, case.Gw)
    u = torch.rand(3, 2, generator=gen) * 0.45 + 0.8
    s[b, :, 0, j, i] = torch.logit(torch.tensor(box[0] - i).clamp(0.02, 0.98))
    s[b, :, 1, j, i] = torch.logit(torch.tensor(box[1] - j).clamp(0.02, 0.98))
    s[b, :, 2, j, i], s[b, :, 3, j, i] = torch.log(box[2] * u[:, 0] / an[:, 0]), torch.log(box[3] * u[:, 1] / an[:, 1])


def place(case, r, seed):
    """every cell within r pixels of a real label's cell predicts that label (predict above); the logits are then rounded to the dtype"""
    real, g = label_boxes(case, case.targets)
    gen = torch.Generator().manual_seed(seed)
    for b, t in real.nonzero().tolist():
        box = g[b, t].tolist()
        for j in range(max(int(box[1]) - r, 0), min(int(box[1]) + r, case.Gh - 1) + 1):
            for i in range(max(int(box[0]) - r, 0), min(int(box[0]) + r, case.Gw - 1) + 1):
                predict(case, b, j, i, box, gen)
    case.sample = rnd(case.dt, case.sample)


#        B  C  Gh Gw T  Cpad ldc  ldd  gscale thr seed
SHAPES = {"plain": (2, 1, 5, 7, 6, 24, None, None, None, 0.3, 1), "strided": (2, 80, 4, 5, 4, 256, 264, 272, 0.25, 0.3, 2),
          "many-rows": (1, 1, 4, 4, None, 24, None, None, None, 0.3, 3), "none": (2, 1, 5, 7, 6, 24, None, None, None, 0.99, 1),
          "all": (1, 1, 2, 2, 1, 24, None, None, None, 0.3, 5), "clamped": (2, 1, 5, 7, 6, 24, None, None, None, 0.3, 6),
          "excluded": (2, 1, 8, 7, 5, 24, None, None, 2.0, 0.3, 7), "two-slabs": (3, 1, 10, 11, 8, 24, None, None, None, 0.3, 8)}


def build(name, dt):
    B, C, Gh, Gw, T, Cpad, ldc, ldd, gscale, thr, seed = SHAPES[name]
    T = T or _lib.ign_lib().yolo_ign_rows_per_pass() + 3
    c = YoloCase(B, C, Gh, Gw, T, dt, 32, seed=seed, min_real=min(T, 3))
    real = label_boxes(c, c.targets)[0][..., None]
    c.targets[..., 3:] = torch.where(real, 0.2 + 1.5 * c.targets[..., 3:], c.targets[..., 3:])      # labels 1 to 3.5 cells wide
    if name == "many-rows":        # three real rows in the first pass, padding up to it, the fourth label in the LAST pass
        c.targets[:] = 0
        c.targets[0, :3, 1:] = torch.tensor([[0.125, 0.125, 0.15, 0.15], [0.8, 0.2, 0.3, 0.4], [0.125, 0.875, 0.15, 0.15]])
        c.targets[0, T - 2, 1:] = torch.tensor([0.7, 0.7, 0.45, 0.4])
    elif name == "all":            # one label over the whole 2x2 grid and every cell predicting it: no negative is left
        c.targets[0, 0] = torch.tensor([0, 0.5, 0.5, 1.0, 1.0])
    place(c, 2 if name == "all" else 1, seed)
    if name == "plain":            # a cell of image 1 beside the cell of image 0's first label predicts THAT label: it must stay a negative
        box = label_boxes(c, c.targets)[1][0, 0].tolist()
        predict(c, 1, int(box[1]), int(box[0]) - 1 if int(box[0]) > 0 else 1, box, torch.Generator().manual_seed(seed))
    elif name == "clamped":        # a huge predicted box (exp clamps at 20) and a label of zero width, which stays a real row
        c.sample.view(B, 3, c.attrs, Gh, Gw)[0, :, 2:4, 0, 0] = 30.0
        c.targets[0, 0, 3] = 0.0
    c.sample = rnd(dt, c.sample)
    return c, Cpad, ldc, ldd, gscale, thr


def read_mask(iws, B, Gh, Gw):
    """the workspace's bit mask -> bool [B,3,Gh,Gw]: bit k of word w of an image is its cell q = 64 w + k, pixel-major, anchor-minor"""
    per = 3 * Gh * Gw
    bits = np.unpackbits(iws[16:].cpu().numpy().reshape(B, -1), axis=1, bitorder="little")
    assert bits.shape[1] == -(-per // 256) * 256 and not bits[:, per:].any()
    return torch.from_numpy(bits[:, :per].reshape(B, Gh, Gw, 3).astype(bool)).permute(0, 3, 1, 2)


@DT
@pytest.mark.parametrize("name", list(SHAPES))
def test_ignore_rule_against_float64(name, dt):
    """MI355X: worst err / max(e32, 4 u scale) = 1.26 (8 allowed; many-rows fp32, loss); the smallest distance of a best IoU to thr in any
    case is 1.4e-3 (two-slabs bf16), 14 times the band"""
    case, Cpad, ldc, ldd, gscale, thr = build(name, dt)
    B, C, Gh, Gw, tag = case.B, case.C, case.Gh, case.Gw, f"{name} {'bf16' if dt else 'fp32'}"
    ign, iou, pos, neg = ign_ref(case, thr, name in ("none", "all"))
    keep = neg & ~ign
    n, left = int(ign.sum()), int(keep.sum())
    if name == "plain":            # some negative of image 1 overlaps a label of image 0 by more than thr, none of its own
        assert bool((keep[1] & (ious(case, case.targets.flip(0)).max(-1).values[1] > thr + BAND)).any())
    elif name == "many-rows":      # some cell is ignored through the row of the last pass alone
        assert bool((ign & (iou[..., :-3].max(-1).values < thr) & (iou[..., -2] > thr)).any())
    elif name == "excluded":       # some unowned cell of an excluded pixel overlaps a label by more than thr: not a negative, not counted
        assert bool((~pos & ~neg & (iou.max(-1).values > thr)).any())
    assert (n == 0) == (name == "none") and (left == 0) == (name == "all")

    K, L, up = _lib.ign_lib(), _lib.lib(), 1.0 if gscale is None else gscale
    out7, dl, ws, (lg, tg, an) = run_train(case, Cpad, ldc=ldc, ldd=ldd, gscale=gscale)             # the head alone, its gradient included
    before7, before, ws0 = out7.clone(), dl.full.clone(), ws.clone()
    iws = torch.zeros(int(K.yolo_ign_workspace_bytes(B, 3, Gh, Gw)), dtype=torch.uint8, device="cuda")
    ign_out = torch.zeros(2, device="cuda")
    gs = torch.tensor([gscale], device="cuda") if gscale is not None else None
    K.check(K.yolo_ign_loss(dt, lg.data_ptr(), ldc or Cpad, tg.data_ptr(), an.data_ptr(), B, case.T, 3, C, Gh, Gw, thr, NOOBJ, ws.data_ptr(),
                            iws.data_ptr(), out7.data_ptr(), ign_out.data_ptr(), st()), "yolo_ign_loss")
    L.check(L.yolo_head_grad(dt, lg.data_ptr(), ldc or Cpad, dl.ptr, ldd or Cpad, Cpad, tg.data_ptr(), an.data_ptr(), *case.geo(), ws.data_ptr(),
                             P(gs), st()), "yolo_head_grad")
    K.check(K.yolo_ign_grad(dt, dl.ptr, ldd or Cpad, Cpad, B, 3, C, Gh, Gw, iws.data_ptr(), P(gs), st()), "yolo_ign_grad")
    sync()

    assert torch.equal(read_mask(iws, B, Gh, Gw), ign), f"{tag}: mask"
    assert ign_out.tolist() == [n, left] and not bool(iws[:16].any()), f"{tag}: n, nN' or the sums left behind"
    acc0, acc, ints = head_counts(ws0, B, 3, Gh, Gw), head_counts(ws, B, 3, Gh, Gw), ws.numel() - 64
    raw, was = dl.full.view(ITYPE[dt]).cpu(), before.view(ITYPE[dt]).cpu()
    if n == 0:
        assert torch.equal(ws, ws0) and torch.equal(out7.view(torch.int32), before7.view(torch.int32)) and torch.equal(raw, was), tag
        return
    other = [0, 1, 2, 3, 4, 6]
    assert torch.equal(ws[:ints], ws0[:ints]) and torch.equal(acc[other], acc0[other]) and float(acc[7]) == left, f"{tag}: head workspace"
    assert torch.equal(out7[1:6].view(torch.int32), before7[1:6].view(torch.int32)), f"{tag}: another part changed"

    M, conf = B * Gh * Gw, torch.zeros(B, Gh, Gw, dl.ld, dtype=torch.bool)
    for a in range(3):
        conf[..., a * case.attrs + 4] = neg[:, a]                                                    # the conf words of the negatives
    full = torch.zeros(dl.full.shape, dtype=torch.bool)
    full[:M] = conf.view(M, dl.ld)
    assert torch.equal(raw[~full], was[~full]), f"{tag}: a word outside the conf words of the negatives changed"
    dl.assert_sentinel_intact()
    g = dl.full[:M].float().cpu().double().view(B, Gh, Gw, dl.ld)
    got = torch.stack([g[..., a * case.attrs + 4] for a in range(3)], 1)
    assert bool((got[ign] == 0).all()), f"{tag}: an ignored cell keeps a conf gradient"
    if left == 0:
        assert bool(out7[[0, 6]].isnan().all()) and float(acc[5]) == 0.0 and bool((got[neg] == 0).all()), tag
        return
    (l64, d64), (l32, d32) = (noobj_ref(case, keep, d) for d in (F64, torch.float32))
    (t64, p64, _), (t32, p32, _) = (hr.yolo_train(case.sample, case.anchors_px, C, case.cfg_h, case.targets, d) for d in (F64, torch.float32))
    o = out7.cpu().double()
    compare(f"{tag} loss_noobj", o[6], l64, l32)
    compare(f"{tag} loss", o[0], t64 - p64[5] + l64, t32 - p32[5] + l32)
    compare(f"{tag} conf gradients", got[keep], d64[keep] * up, d32[keep] * up, bf16_store=dt == BF16)


def test_stand_alone_layer():
    """`noobj_ignored`, the no-object part and d loss / d sample: zero at the ignored conf logits, rescaled at the other negatives' and
    the plain layer's bits everywhere else; pred_ignore=0.99 ignores nothing and returns the plain layer's bits"""
    from mdcv.yolo.models import YOLOLayer
    case, _, _, _, _, thr = build("plain", F32)
    ign, _, _, neg = ign_ref(case, thr, False)
    keep, runs = neg & ~ign, []
    for kw in ({}, dict(pred_ignore=0.99), dict(pred_ignore=thr)):
        lay = YOLOLayer(case.anchors_px, 1, case.cfg_h, case.cfg_h, 0.5, "leaky", 2.0, 1.6, 0.1, NOOBJ, **kw)
        s = case.sample.cuda().requires_grad_(True)
        loss, parts = lay(s, case.targets.cuda())
        loss.backward()
        runs.append((loss.detach().cpu(), parts.cpu(), s.grad.cpu().view(case.B, 3, case.attrs, case.Gh, case.Gw)))
    assert all(torch.equal(x, y) for x, y in zip(runs[0], runs[1])) and lay.noobj_ignored.tolist() == [int(ign.sum()), int(keep.sum())]
    (l64, d64), (l32, d32) = (noobj_ref(case, keep, d) for d in (F64, torch.float32))
    compare("layer loss_noobj", runs[2][1][5].double(), l64, l32)
    conf = torch.zeros_like(runs[0][2], dtype=torch.bool)
    conf[:, :, 4] = neg
    assert torch.equal(runs[2][2][~conf], runs[0][2][~conf]) and bool((runs[2][2][:, :, 4][ign] == 0).all())
    compare("layer conf gradients", runs[2][2][:, :, 4][keep].double(), d64[keep], d32[keep])


def test_darknet_with_and_without_the_ignore_rule(monkeypatch):
    """mini.cfg with its weights and recorded batch: pred_ignore=0 builds the launch lists of a model made without the keyword; 0.99
    ignores nothing, so the loss, the parts and every gradient equal the plain model's, with one call more per head and pass; 0.3
    ignores cells in both heads and changes the no-object part alone"""
    from mdcv.yolo.models import Darknet
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    monkeypatch.chdir(os.path.join(golden, "mini"))                                                  # (the cfg names its anchor file relative to itself)
    nets = [Darknet("mini.cfg", 2.0, 1.6, NOOBJ, 0.1, False, precision="fp32", **kw) for kw in ({}, dict(pred_ignore=0.0), dict(pred_ignore=0.99), dict(pred_ignore=0.3))]
    for net in nets:
        net.load_weights("mini.weights", net.get_start_weight_dim())
        net.cuda().train()
    z = np.load(os.path.join(golden, "mini_darknet.npz"))
    x, tg = torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["targets"]).cuda()
    grads = lambda net: torch.cat([p.grad.flatten() for p in net.parameters()])                      # noqa: E731
    (o_plain, _, f_plain, b_plain), g_plain = step(nets[0], x, tg), grads(nets[0])
    (o0, _, f0, b0), (o1, _, f1, b1), g1, (o2, _, _, _) = step(nets[1], x, tg), step(nets[2], x, tg), grads(nets[2]), step(nets[3], x, tg)
    assert (f0, b0) == (f_plain, b_plain) and nets[1].noobj_ignored is None and torch.equal(o0, o_plain)
    assert [n for n, _ in f1].count("mdcv_yolo_ign_loss") == 2 and [n for n, _ in b1].count("mdcv_yolo_ign_grad") == 2
    assert len(f1) == len(f0) + 2 and len(b1) == len(b0) + 2 and torch.equal(o1, o_plain) and torch.equal(g1, g_plain)
    none, some = nets[2].noobj_ignored, nets[3].noobj_ignored
    assert some.is_cuda and some.shape == (2, 2) and bool((none[:, 0] == 0).all()) and bool((some[:, 0] > 0).all())
    assert torch.equal(some.sum(1), none[:, 1]) and torch.equal(o2[1:6], o_plain[1:6]) and float(o2[6]) != float(o_plain[6])
    assert not torch.equal(grads(nets[3]), g_plain)
