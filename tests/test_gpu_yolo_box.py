"""-m gpu: the opt-in box loss of the YOLO head (csrc/yolo_box.hip) against include/mdcv_box.h's formulas in float64 torch autograd, under
test_gpu_heads.py's rule unchanged (`compare`; bf16 half ulp at the magnitude of head + box gradient).  Support is exact, guard bands included."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from mdcv import _lib  # noqa: E402
from test_gpu_heads import F32, BF16, ITYPE, YoloCase, compare, head_counts, hr, rnd, run_train, st, sync  # noqa: E402
from test_gpu_yolo_cls import PAIR, step  # noqa: E402

F64, EPS = torch.float64, 1e-7
MODES = pytest.mark.parametrize("mode", ["giou", "diou", "ciou"])


def owned(case):
    """-> (b, a, j, i) of the owned cells, the owner row's box [N,4] (fp32 products); padding rows take row 0, a later row wins its cell"""
    tg, an = case.targets, hr.scaled_anchors(case.anchors_px, case.stride)
    src = torch.where((tg.sum(2) > 0)[..., None], tg, tg[:, :1].expand_as(tg))
    box = src[..., 1:] * torch.tensor([case.Gw, case.Gh, case.Gw, case.Gh], dtype=torch.float32)
    gt = torch.cat((torch.zeros_like(box[..., :2]), box[..., 2:]), -1)[:, None]
    best = hr.yo.corner_iou_plus1(gt, torch.cat((torch.zeros(3, 2), an), 1)[None, :, None]).argmax(1)
    out = (box[..., 0] >= case.Gw) | (box[..., 1] >= case.Gh)
    own = {(b, int(best[b, t]), int(box[b, t, 1]), int(box[b, t, 0])): box[b, t] for b in range(case.B) for t in range(case.T) if not out[b, t]}
    seen = tg.clone()
    seen[out] = 0                                      # what the oracle may see of a dropped row: one more padding row
    mask = hr.yo.build_targets(seen, an, 3, case.C, case.Gh, case.Gw, 0.5)[0]
    assert sorted(own) == [tuple(c) for c in mask.nonzero().tolist()]
    return tuple(torch.tensor(sorted(own)).T), torch.stack([own[c] for c in sorted(own)])


def box_ref(case, own, mode, k, dtype):
    """-> loss_box, mean IoU, d loss_box / d sample, per-cell IoU as float64 tensors of the values computed in `dtype`; asserts tie-freedom"""
    (b, a, j, i), g = own
    s = case.sample.detach().to(dtype).clone().requires_grad_(True)
    z = s.view(case.B, 3, 5 + case.C, case.Gh, case.Gw)[b, a, :, j, i]
    an = hr.scaled_anchors(case.anchors_px, case.stride).to(dtype)[a]
    px, py = hr.stable_sigmoid(z[:, 0]) + i, hr.stable_sigmoid(z[:, 1]) + j
    pw, ph = torch.exp(z[:, 2].clamp(max=20)) * an[:, 0], torch.exp(z[:, 3].clamp(max=20)) * an[:, 1]
    gx, gy, gw, gh = g.to(dtype).unbind(1)
    pairs, zero = [], torch.zeros_like(px)
    mn = lambda u, v: (pairs.append((u, v)), torch.min(u, v))[1]     # noqa: E731
    mx = lambda u, v: (pairs.append((u, v)), torch.max(u, v))[1]     # noqa: E731
    iw = mx(mn(px + pw / 2, gx + gw / 2) - mx(px - pw / 2, gx - gw / 2), zero)
    ih = mx(mn(py + ph / 2, gy + gh / 2) - mx(py - ph / 2, gy - gh / 2), zero)
    union = pw * ph + gw * gh - iw * ih + EPS
    iou = iw * ih / union
    cw = mx(px + pw / 2, gx + gw / 2) - mn(px - pw / 2, gx - gw / 2)
    ch = mx(py + ph / 2, gy + gh / 2) - mn(py - ph / 2, gy - gh / 2)
    if mode == "giou":
        q = iou - (cw * ch + EPS - union) / (cw * ch + EPS)
    else:
        q = iou - ((px - gx) ** 2 + (py - gy) ** 2) / (cw ** 2 + ch ** 2 + EPS)
        if mode == "ciou":
            v = 4 / math.pi ** 2 * (torch.atan(gw / (gh + EPS)) - torch.atan(pw / (ph + EPS))) ** 2
            q = q - (v / (v - iou + 1 + EPS)).detach() * v
    loss = k * (1 - q).mean()
    loss.backward()
    assert all(bool((u != v).all()) for u, v in pairs), "a min / max pair of the reference ties"
    return loss.detach().double(), iou.mean().detach().double(), s.grad.double(), iou.detach().double()


def put(case, own, px, py, pw, ph):
    (b, a, j, i), _ = own                              # the predicted box of every owned cell becomes (px, py, pw, ph), centre kept in its cell
    an = hr.scaled_anchors(case.anchors_px, case.stride)[a]
    case.sample.view(case.B, 3, 5 + case.C, case.Gh, case.Gw)[b, a, :4, j, i] = torch.stack(
        [torch.logit((px - i).clamp(0.02, 0.98)), torch.logit((py - j).clamp(0.02, 0.98)), torch.log(pw / an[:, 0]), torch.log(ph / an[:, 1])], 1)
    case.sample = rnd(case.dt, case.sample)


def build(name, dt):
    B, C, Gh, Gw, T, Cpad = {"strided": (3, 4, 13, 19, 6, 32), "collide": (2, 1, 13, 13, 5, 24),
                             "grid-stride": (3, 1, 13, 13, 2800, 24)}.get(name, (2, 1, 13, 13, 4, 24))   # grid-stride: 8400 rows > 32 * 256
    c = YoloCase(B, C, Gh, Gw, T, dt, 32, seed=len(name) + 3, min_real=min(T, 4))
    ldc, ldd, gscale = (40, 48, 0.25) if name == "strided" else (None, None, None)   # 27 channels, NaN in the pad channels, ldd != Cpad
    hyper = (0.5, 2.0, 1.6, 0.1, 25.0) if name == "alive" else (0.5, 0.0, 0.0, 0.1, 25.0)   # alive: the MSE gradients share the channels
    c.geo = lambda: (c.B, c.T, 3, c.C, c.Gh, c.Gw) + hyper
    if name == "disjoint":
        c.targets[..., 3:] *= 0.1                                                # labels at most 0.39 cells wide ...
    elif name == "zero-width":
        c.targets[0, 0, 3] = 0.0
    elif name == "collide":        # rows 1, 2: one cell and anchor, row 2 owns it; row 3 padding (row 0 again); row 4 dropped (cx = 1)
        c.targets[0] = torch.tensor([[0, 0.2, 0.8, 0.1, 0.2], [0] + PAIR[0], [0] + PAIR[1], [0, 0, 0, 0, 0], [0, 1.0, 0.5, 0.1, 0.1]])
    own = owned(c)
    gx, gy, gw, gh = own[1].unbind(1)
    odd = torch.arange(len(gx)) % 2
    if name == "near":             # the label box perturbed by 5-20 % per coordinate: IoU 0.5-0.8
        u = (torch.rand(4, len(gx), generator=torch.Generator().manual_seed(5)) * 0.15 + 0.05) * (1 - 2 * odd)
        put(c, own, gx + u[0] * gw, gy + u[1] * gh, gw * (1 + u[2]), gh * (1 + u[3]))
    elif name == "disjoint":       # ... and a 0.2-wide prediction 0.4 cells beside the label's centre: no overlap in x
        put(c, own, gx + torch.where(gx - gx.floor() < 0.5, 0.4, -0.4), gy + 0.1 * gh, torch.full_like(gw, 0.2), 1.3 * gh)
    elif name == "inside":         # even cells: prediction strictly inside the label (IoU 1/4); odd cells: strictly around it (1/2.56)
        put(c, own, gx + 0.05 * gw, gy - 0.05 * gh, gw * (0.5 + 1.1 * odd), gh * (0.5 + 1.1 * odd))
    elif name == "clamped":
        c.sample.view(B, 3, 5 + C, Gh, Gw)[own[0][0][0], own[0][1][0], 2, own[0][2][0], own[0][3][0]] = 25.0
    return c, Cpad, ldc, ldd, gscale, own


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@MODES
@pytest.mark.parametrize("name", ["plain", "near", "disjoint", "inside", "clamped", "zero-width", "collide", "strided", "grid-stride", "alive"])
def test_box_loss_and_grad_against_float64(name, mode, dt):
    """MI355X: worst err / max(e32, 4 u scale) = 0.20 (8 allowed; near, mean IoU and dlogits); bf16 dlogits against the flat 2^-9 |ref|: 1.89.
    The stand-alone layer below: 0.39 (diou, d sample)."""
    case, Cpad, ldc, ldd, gscale, own = build(name, dt)
    K, up, tag = _lib.box_lib(), 1.0 if gscale is None else gscale, f"{name} {mode} {'bf16' if dt else 'fp32'}"
    (loss, miou, ds, iou), (loss32, miou32, ds32, _) = (box_ref(case, own, mode, 0.7, d) for d in (F64, torch.float32))
    out7, dl, ws, (lg, tg, an) = run_train(case, Cpad, ldc=ldc, ldd=ldd, gscale=gscale)
    before7, before = out7.clone(), dl.full.clone()
    bws, box_out = torch.zeros(int(K.yolo_box_workspace_bytes()), dtype=torch.uint8, device="cuda"), torch.zeros(2, device="cuda")
    gs = torch.tensor([gscale], device="cuda") if gscale is not None else None
    geo = (case.B, case.T, 3, case.C, case.Gh, case.Gw, 0.5, _lib.BOX_MODES[mode], 0.7)
    K.check(K.yolo_box_loss(dt, lg.data_ptr(), ldc or Cpad, tg.data_ptr(), an.data_ptr(), *geo, ws.data_ptr(), bws.data_ptr(),
                            out7.data_ptr(), box_out.data_ptr(), st()), "yolo_box_loss")
    K.check(K.yolo_box_grad(dt, lg.data_ptr(), ldc or Cpad, dl.ptr, ldd or Cpad, Cpad, tg.data_ptr(), an.data_ptr(), *geo, ws.data_ptr(),
                            gs.data_ptr() if gs is not None else None, st()), "yolo_box_grad")
    sync()
    compare(f"{tag} loss_box", box_out.cpu().double()[0], loss, loss32)
    compare(f"{tag} mean iou", box_out.cpu().double()[1], miou, miou32)
    same = lambda x, y: torch.allclose(x, y, rtol=0, atol=0, equal_nan=True)   # noqa: E731  (== ; the head's parts may be NaN)
    assert same(out7[0], before7[0] + box_out[0]) and same(out7[1:], before7[1:]) and not bool(bws.any()), f"{tag}: out7 / workspace"
    assert float(head_counts(ws, case.B, 3, case.Gh, case.Gw)[6]) == len(iou)                        # every owned cell once
    (b, a, j, i), M = own[0], case.B * case.Gh * case.Gw
    sel = torch.zeros(case.B, case.Gh, case.Gw, dl.ld, dtype=torch.bool)                             # channels 0..3 of owned cells
    for k in range(4):
        sel[b, j, i, a * case.attrs + k] = True
    full = torch.zeros(dl.full.shape, dtype=torch.bool)
    full[:M] = sel.view(M, dl.ld)
    raw, was = dl.full.view(ITYPE[dt]).cpu(), before.view(ITYPE[dt]).cpu()
    assert torch.equal(raw[~full], was[~full]), f"{tag}: a word outside channels 0..3 of owned cells changed"
    dl.assert_sentinel_intact()
    pick = lambda t: t.permute(0, 2, 3, 1)[sel[..., :case.ch]].view(-1, 4)                           # noqa: E731
    rows = lambda t: t[:M].float().view(case.B, case.Gh, case.Gw, -1)[..., :case.ch][sel[..., :case.ch]].cpu().double().view(-1, 4)   # noqa: E731
    got, head = rows(dl.full), rows(before)
    compare(f"{tag} dlogits", got, head + pick(ds) * up, head + pick(ds32) * up, bf16_store=dt == BF16)
    assert bool(head.any()) == (name == "alive")
    if name == "disjoint":         # plain IoU has no gradient here; these have, in x and w of every cell (the enclosing box, the distance)
        assert not bool(iou.any()) and bool((pick(ds)[:, [0, 2]] != 0).all())
    elif name == "clamped":        # one cell's w channel: the value took exp(20) (the loss above) and the gradient is exactly 0
        dead = pick(ds)[:, 2] == 0
        assert int(dead.sum()) == 1 and float(got[dead, 2]) == 0.0


@MODES
def test_stand_alone_layer(mode):
    """`loss_box`, `box_iou` and the x/y/w/h part of d loss / d sample (beside the MSE gradients); elsewhere the plain layer's bits"""
    from mdcv.yolo.models import YOLOLayer
    case, _, _, _, _, own = build("near", F32)
    (loss, miou, ds, _), (loss32, miou32, ds32, _) = (box_ref(case, own, mode, 0.7, d) for d in (F64, torch.float32))
    grads = []
    for kw in ({}, dict(box_loss=0.7, box_mode=mode)):
        lay = YOLOLayer(case.anchors_px, 1, case.cfg_h, case.cfg_h, 0.5, "leaky", 2.0, 1.6, 0.1, 25.0, **kw)
        s = case.sample.cuda().requires_grad_(True)
        lay(s, case.targets.cuda())[0].backward()
        grads.append(s.grad.cpu().double())
    compare(f"layer {mode} loss_box", lay.loss_box.cpu().double()[0], loss, loss32)
    compare(f"layer {mode} box_iou", lay.box_iou.cpu().double()[0], miou, miou32)
    live = ds != 0
    assert torch.equal(grads[1][~live], grads[0][~live])
    compare(f"layer {mode} dsample", grads[1][live], grads[0][live] + ds[live], grads[0][live] + ds32[live])


@MODES
def test_darknet_with_and_without_the_box_loss(mode, monkeypatch):
    """tiny cfg: box_loss=0 builds the launch lists of a model made without the keyword; with it each head adds one loss and one grad
    call, the totals differ by model.loss_box (three fp32 additions in another order: 4 ulp), the six parts are bit-equal.  MDCV_GRAPH=1:
    warm run + capture and two replays, each on other labels, equal the eager step.  With the class loss on too the total gains both."""
    from mdcv.yolo.models import Darknet
    monkeypatch.chdir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mini"))    # (the cfg names its anchor file relative to itself)
    on = dict(box_loss=1.0, box_mode=mode)
    nets = [Darknet("mini_tiny.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32", **kw).cuda().train()
            for kw in ({}, dict(on, box_loss=0.0), on, on, dict(on, cls_loss=1.0))]
    for n in nets[1:]:
        n.load_state_dict(nets[0].state_dict())
    nets[3].use_graph = True
    g = torch.Generator().manual_seed(3)
    x, tg = torch.rand(2, 3, 64, 64, generator=g).cuda(), hr.yolo_targets(2, 5, g).cuda()
    (o_plain, _, f_plain, b_plain), (o0, _, f0, b0), (o1, _, f1, b1), (o2, _, _, _) = (step(nets[k], x, tg) for k in (0, 1, 2, 4))
    assert (f0, b0) == (f_plain, b_plain) and nets[1].loss_box is None and nets[1].box_iou is None and torch.equal(o0, o_plain)
    assert [n for n, _ in f1].count("mdcv_yolo_box_loss") == 2 and [n for n, _ in b1].count("mdcv_yolo_box_grad") == 2
    assert len(f1) == len(f0) + 3 and len(b1) == len(b0) + 2 and torch.equal(o1[1:], o0[1:])
    lb, bi, ulp = nets[2].loss_box, nets[2].box_iou, 2.0 ** -23
    assert lb.is_cuda and lb.shape == (1,) and bi.is_cuda and bi.shape == (1,) and float(lb) > 0 and 0 < float(bi) <= 1
    assert abs((float(o1[0]) - float(o0[0])) - float(lb)) <= 4 * ulp * abs(float(o1[0]))
    both = float(nets[4].loss_box) + float(nets[4].loss_cls)
    assert torch.equal(nets[4].loss_box, lb) and abs((float(o2[0]) - float(o0[0])) - both) <= 8 * ulp * abs(float(o2[0]))
    for it in range(3):
        (oe, ge, _, _), (og, gg, _, _) = (step(n, x, tg) for n in nets[2:4])
        assert torch.equal(oe, og) and torch.equal(nets[2].loss_box, nets[3].loss_box) and torch.equal(nets[2].box_iou, nets[3].box_iou), it
        assert float((ge - gg).abs().max()) <= 1e-6 * float(ge.abs().max()), it
        tg = hr.yolo_targets(2, 5, g).cuda()
