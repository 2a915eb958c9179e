"""-m gpu: the opt-in class loss of the YOLO head, csrc/yolo_cls.hip (mdcv_yolo_cls_loss / _grad, include/mdcv_cls.h), through the C ABI and
through Darknet, against a float64 reference: a few lines of torch on oracle.yolo_oracle.build_targets' `mask` and `tcls`.

Tolerances are test_gpu_heads.py's rule: max |kernel - ref| <= head_refs.bound(max |r32 - ref|, max |ref|), r32 the reference in float32,
plus the bf16 half ulp per element for bf16 dlogits.  Support is exact: every word of the dlogits buffer outside the class channels of
owned cells keeps the bits mdcv_yolo_head_grad wrote (guard bands included), and out7[1..6] keep theirs.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from mdcv import _lib  # noqa: E402
from test_gpu_heads import F32, BF16, ITYPE, YoloCase, compare, head_counts, hr, run_train, st, sync  # noqa: E402

F64 = torch.float64
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = pytest.mark.parametrize("mode", ["ce", "bce"])
DT = pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
PAIR = ([8.2 / 13, 3.3 / 13, 0.10, 0.10], [8.7 / 13, 3.6 / 13, 0.11, 0.09])      # two boxes of one cell (3, 8) and one best anchor


def cls_ref(case, targets, mode, cls_loss, dtype):
    """-> loss_cls (0-d), d loss_cls / d sample [B, A(5+C), Gh, Gw], mask, tcls[mask]; float64 tensors of the values computed in `dtype`"""
    B, C, Gh, Gw = case.B, case.C, case.Gh, case.Gw
    s = case.sample.detach().to(dtype).clone().requires_grad_(True)
    p = hr.stable_sigmoid(s.view(B, 3, 5 + C, Gh, Gw).permute(0, 1, 3, 4, 2)[..., 5:])
    out = hr.yo.build_targets(targets, hr.scaled_anchors(case.anchors_px, case.stride), 3, C, Gh, Gw, 0.5)
    mask, tcls = torch.as_tensor(out[0]).bool(), torch.as_tensor(out[7])
    if mode == "ce":
        term = F.cross_entropy(p[mask], torch.from_numpy(np.argmax(tcls[mask].numpy(), 1)))
    else:
        term = F.binary_cross_entropy(p[mask], tcls[mask].to(dtype))
    loss = (cls_loss / B) * term
    loss.backward()
    return loss.detach().double(), s.grad.double(), mask, tcls[mask]


def run_cls(case, mode, cls_loss, Cpad, ldc=None, ldd=None, gscale=None):
    """head train (loss + gradient), then the two class entries behind it -> everything the checks need"""
    K = _lib.cls_lib()
    out7, dl, ws, (lg, tg, an) = run_train(case, Cpad, ldc=ldc, ldd=ldd, gscale=gscale)
    before7, before = out7.clone(), dl.full.clone()
    cws = torch.zeros(int(K.yolo_cls_workspace_bytes()), dtype=torch.uint8, device="cuda")
    cls_out = torch.zeros(1, device="cuda")
    gs = torch.tensor([gscale], device="cuda") if gscale is not None else None
    geo = (case.B, case.T, 3, case.C, case.Gh, case.Gw, 0.5, _lib.CLS_MODES[mode], cls_loss)
    K.check(K.yolo_cls_loss(case.dt, lg.data_ptr(), ldc or Cpad, tg.data_ptr(), an.data_ptr(), *geo, ws.data_ptr(), cws.data_ptr(),
                            out7.data_ptr(), cls_out.data_ptr(), st()), "yolo_cls_loss")
    K.check(K.yolo_cls_grad(case.dt, lg.data_ptr(), ldc or Cpad, dl.ptr, ldd or Cpad, Cpad, tg.data_ptr(), an.data_ptr(), *geo, ws.data_ptr(),
                            gs.data_ptr() if gs is not None else None, st()), "yolo_cls_grad")
    sync()
    return dict(out7=out7, before7=before7, dl=dl, before=before, cls=cls_out, err=int(cws.view(torch.int32)[_lib.CLS_ERR_WORD]), ws=ws)


def check_cls(tag, case, r, refs, gscale=None, e32_free=False):
    (loss, ds, mask, _), (loss32, ds32, _, _) = refs
    none = lambda t: None if e32_free else t        # noqa: E731
    compare(f"{tag} loss_cls", r["cls"].cpu().double()[0], loss, none(loss32))
    same = lambda a, b: torch.allclose(a, b, rtol=0, atol=0, equal_nan=True)   # noqa: E731  (== ; the head's no-object part is NaN when no cell is left for it)
    assert same(r["out7"][0], r["before7"][0] + r["cls"][0]), f"{tag}: out7[0] did not gain the class scalar"
    assert same(r["out7"][1:], r["before7"][1:]), f"{tag}: the six parts changed"
    dl, M, attrs = r["dl"], case.B * case.Gh * case.Gw, case.attrs
    sel = torch.zeros(case.B, case.Gh, case.Gw, dl.ld, dtype=torch.bool)                   # class channels of owned cells
    for a in range(3):
        sel[..., a * attrs + 5:(a + 1) * attrs] = mask[:, a, :, :, None]
    full = torch.zeros(dl.full.shape, dtype=torch.bool)
    full[:M] = sel.view(M, dl.ld)
    raw, was = dl.full.view(ITYPE[case.dt]).cpu(), r["before"].view(ITYPE[case.dt]).cpu()
    assert torch.equal(raw[~full], was[~full]), f"{tag}: a word outside the class channels of owned cells changed"
    dl.assert_sentinel_intact()
    assert not bool(was[full].any()), "the head wrote zeros there"
    up = 1.0 if gscale is None else gscale
    pick = lambda t: t.permute(0, 2, 3, 1)[sel[..., :case.ch]]                             # noqa: E731
    got = dl.rows(0, M).view(case.B, case.Gh, case.Gw, -1)[..., :case.ch][sel[..., :case.ch]]
    compare(f"{tag} dlogits", got, pick(ds) * up, None if e32_free else pick(ds32) * up, bf16_store=case.dt == BF16)
    return got


def spread_classes(case, seed):                        # ids over all C classes in the real rows (YoloCase draws ids below 3)
    g = torch.Generator().manual_seed(seed)
    real = case.targets.sum(-1) > 0
    case.targets[..., 0][real] = torch.randint(0, case.C, (int(real.sum()),), generator=g).float()


def build(name, dt):
    """-> case, Cpad, ldc, ldd, gscale, targets the reference sees (None: the case's own), e32_free, err word expected"""
    shapes = {"C1": (2, 1, 13, 13, 4, 24), "C4-13x19": (3, 4, 13, 19, 6, 32), "C80": (2, 80, 13, 13, 8, 256), "C130": (1, 130, 7, 7, 3, 408),
              "collide": (2, 4, 13, 13, 5, 32), "T1-B1": (1, 4, 13, 13, 1, 32), "blocks": (3, 4, 13, 13, 50, 32),
              "grid-stride": (3, 4, 13, 13, 1400, 32), "saturated": (2, 4, 13, 13, 6, 32)}
    # C1: softmax over one class, ce exactly 0.  C80 / C130: second lane round / third round (classes from 128 up are re-read).  blocks: 38
    # blocks.  grid-stride: 4200 rows > 4 * 1024 blocks, 22 scan chunks of 64 rows per image.
    B, C, Gh, Gw, T, Cpad = shapes.get(name, (1, 4, 13, 13, 3, 32))
    c = YoloCase(B, C, Gh, Gw, T, dt, 32, seed=len(name) + C, min_real=min(T, 4))
    spread_classes(c, 7)
    ldc, ldd, gscale, seen, e32_free, err = None, None, None, None, False, 0
    if name == "C4-13x19":                             # 27 channels: NaN in the pad channels of a 40-wide row, ldd != Cpad, gscale
        ldc, ldd, gscale = 40, 48, 0.25
    elif name == "collide":                            # rows 1, 2: one cell and anchor, classes 3 and 1; row 3 padding; row 4 dropped (cx = 1)
        c.targets[0] = torch.tensor([[2, 0.2, 0.8, 0.1, 0.2], [3] + PAIR[0], [1] + PAIR[1], [0, 0, 0, 0, 0], [2, 1.0, 0.5, 0.1, 0.1]])
        seen = c.targets.clone()
        seen[0, 4] = 0                                 # what the reference may see: the dropped row as one more padding row (row 0 again)
    elif name == "saturated":                          # class logits at +-60 in owned cells: sigmoid rounds to 1, log(1 - p) takes the clamp;
        s = c.sample.view(2, 3, 9, 13, 13)             # both sides fp32, bound 8 * 4 u scale, as test_yolo_saturated_logits
        for n, (b, a, j, i) in enumerate(c.masks()[0].nonzero().tolist()[:4]):
            s[b, a, 5:, j, i] = torch.tensor([60.0, -60.0, 60.0, -60.0]) * (1 if n % 2 == 0 else -1)
        e32_free = True
    elif name.startswith("id"):                        # row 2 shares cell and anchor with row 1 (class 1); an id >= C or <= -1 sets the err word
        bad, as_id, err = {"id4": (4.0, 1, 1), "id-2": (-2.0, 1, 1), "id-0.5": (-0.5, 0, 0), "id3.9": (3.9, 3, 0)}[name]
        c.targets[0] = torch.tensor([[2, 0.2, 0.8, 0.1, 0.2], [1] + PAIR[0], [bad] + PAIR[1]])
        seen = c.targets.clone()                       # ... and contributes nothing: the result of the cell's other ids alone; ids in (-1, 0)
        seen[0, 2, 0] = as_id                          # and (3, 4) truncate to 0 and 3 and are good
    return c, Cpad, ldc, ldd, gscale, seen, e32_free, err


CASES = ["C1", "C4-13x19", "C80", "C130", "collide", "T1-B1", "blocks", "grid-stride", "saturated", "id4", "id-2", "id-0.5", "id3.9"]


@DT
@MODES
@pytest.mark.parametrize("name", CASES)
def test_cls_loss_and_grad_against_float64(name, mode, dt):
    """Class scalar, the increment of out7[0], out7[1..6] unchanged, dlogits values and exact support, the err word -- per case of `build`.
    MI355X: worst err / max(e32, 4 u scale) = 1.2 (8 allowed); bf16 dlogits against the flat 2^-9 |ref|: 1.96."""
    case, Cpad, ldc, ldd, gscale, seen, e32_free, err = build(name, dt)
    seen = case.targets if seen is None else seen
    refs = [cls_ref(case, seen, mode, 0.7, d) for d in ((torch.float32,) * 2 if e32_free else (F64, torch.float32))]
    r = run_cls(case, mode, 0.7, Cpad, ldc, ldd, gscale)
    got = check_cls(f"{name} {mode} {'bf16' if dt else 'fp32'}", case, r, refs, gscale, e32_free)
    mask, sets = refs[0][2], refs[0][3]
    assert r["err"] == err and float(head_counts(r["ws"], case.B, 3, case.Gh, case.Gw)[6]) == float(mask.sum())   # every owned cell once
    if name == "C1":
        assert (float(r["cls"]) == 0.0 and not bool(got.any())) if mode == "ce" else (float(r["cls"]) > 0.0 and bool(got.any()))
    if name == "collide":
        k = [n for n, (b, a, j, i) in enumerate(mask.nonzero().tolist()) if (b, j, i) == (0, 3, 8)]
        assert len(k) == 1 and sets[k[0]].tolist() == [0, 1, 0, 1]                                   # multi-hot {1, 3}, c* = 1, one cell


@MODES
def test_stand_alone_layer(mode):
    """on an NCHW sample: `loss_cls` and the class part of d loss / d sample against the reference; elsewhere the gradient is that of the
    layer without the class loss, bit for bit.  A bad class id raises at once."""
    from mdcv.yolo.models import YOLOLayer
    case = build("T6", F32)[0]
    (loss, ds, _, _), (loss32, ds32, _, _) = (cls_ref(case, case.targets, mode, 0.7, d) for d in (F64, torch.float32))
    grads = []
    for kw in ({}, dict(cls_loss=0.7, cls_mode=mode)):
        lay = YOLOLayer(case.anchors_px, 4, case.cfg_h, case.cfg_h, 0.5, "leaky", 2.0, 1.6, 0.1, 25.0, **kw)
        s = case.sample.cuda().requires_grad_(True)
        lay(s, case.targets.cuda())[0].backward()
        grads.append(s.grad.cpu().double())
    compare(f"layer {mode} loss_cls", lay.loss_cls.cpu().double()[0], loss, loss32)
    live = ds != 0
    assert torch.equal(grads[1][~live], grads[0][~live]) and not bool(grads[0][live].any())
    compare(f"layer {mode} dsample", grads[1][live], ds[live], ds32[live])
    case.targets[0, 0, 0] = 4.0
    with pytest.raises(IndexError, match="class id"):
        lay(case.sample.cuda(), case.targets.cuda())


def step(net, x, tg):
    net.zero_grad(set_to_none=True)
    out = net(x, tg)
    out[0].backward()
    sync()
    head = [m[0] for d, m in zip(net.module_defs, net.module_list) if d.get("filters") == "preyolo"][-1]
    plan = next(reversed(net._plans.values()))
    names = lambda lst: [(getattr(fn, "__name__", str(fn)), len(args)) for fn, args in lst]      # noqa: E731
    return torch.stack(out).detach(), head.weight.grad.clone(), names(plan.fwd), names(plan.bwd)


@MODES
def test_darknet_with_and_without_the_class_loss(mode, tmp_path):
    """tiny cfg, 4 classes: the totals differ by model.loss_cls (three fp32 additions in another order: 4 ulp), the six parts are bit-equal,
    the class rows of the last head conv's weight gradient are exact zeros without the class loss and alive with it; cls_loss=0 builds the
    launch lists of a model made without the keyword.  MDCV_GRAPH=1: warm run + capture and two replays, each on other labels, equal the
    eager step bit for bit.  A class id of 4 raises IndexError one step late, naming it."""
    from mdcv.yolo.models import Darknet
    txt = open(os.path.join(G, "mini", "mini_tiny.cfg")).read().replace("classes=1", "classes=4")
    cfg = os.path.join(str(tmp_path), "tiny4.cfg")
    open(cfg, "w").write(txt.replace("train_uri=dataset/train.csv", "train_uri=" + os.path.join(G, "mini", "dataset", "train.csv")))
    on = dict(cls_loss=1.0, cls_mode=mode)
    nets = [Darknet(cfg, 2.0, 1.6, 25.0, 0.1, False, precision="fp32", **kw).cuda().train() for kw in ({}, dict(on, cls_loss=0.0), on, on)]
    for n in nets[1:]:
        n.load_state_dict(nets[0].state_dict())
    nets[3].use_graph = True
    g = torch.Generator().manual_seed(3)
    x, tg = torch.rand(2, 3, 64, 64, generator=g).cuda(), hr.yolo_targets(2, 5, g, cls_hi=4).cuda()
    (o_plain, _, f_plain, b_plain), (o0, g0, f0, b0), (o1, g1, f1, b1) = (step(n, x, tg) for n in nets[:3])
    assert (f0, b0) == (f_plain, b_plain) and nets[1].loss_cls is None and torch.equal(o0, o_plain)
    assert [n for n, _ in f1].count("mdcv_yolo_cls_loss") == 2 and [n for n, _ in b1].count("mdcv_yolo_cls_grad") == 2
    assert len(f1) == len(f0) + 3 and len(b1) == len(b0) + 2 and torch.equal(o1[1:], o0[1:])
    lc = nets[2].loss_cls
    assert lc.is_cuda and lc.shape == (1,) and float(lc) > 0
    assert abs((float(o1[0]) - float(o0[0])) - float(lc)) <= 4 * 2.0 ** -23 * abs(float(o1[0]))
    rows = torch.tensor([a * 9 + 5 + c for a in range(3) for c in range(4)])
    assert not bool(g0[rows].any()) and bool(g1[rows].flatten(1).any(1).all())
    for it in range(3):
        (oe, ge, _, _), (og, gg, _, _) = (step(n, x, tg) for n in nets[2:])
        assert torch.equal(oe, og) and torch.equal(nets[2].loss_cls, nets[3].loss_cls), it
        assert float((ge - gg).abs().max()) <= 1e-6 * float(ge.abs().max()), it
        tg = hr.yolo_targets(2, 5, g, cls_hi=4).cuda()
    bad = tg.clone()
    bad[1, 0, 0] = 4.0
    nets[2](x, bad)
    nets[0](x, bad)                                    # without the class loss nobody looks at class ids, as before
    with pytest.raises(IndexError, match="class id"):
        nets[2](x, tg)
    nets[2](x, tg), nets[0](x, tg)
