"""Darknet cfg sections -> launch-plan entries, one unit per section kind.

`analyse` is the host-only graph analysis (who uses what, shapes, zero-copy concat layout).  Each `lower_<kind>(cx, i, d)` appends
the forward launches of section i to `cx.plan.fwd` and returns a record whose `backward(plan)` -- directly beneath it -- appends the
mirrored launches to `plan.bwd`; Darknet._build_plan (yolo/models.py) drives them through `FORWARD`.
"""
from collections import namedtuple
from dataclasses import dataclass

import torch

from .. import _lib, netplan
from ..engine import Act, TNode, ConvSpec, BnSpec, pad8, ACT_NONE, ACT_LEAKY, ACT_RELU


def _res(i, v):                                              # cfg layer reference -> absolute module index
    return i + v if v < 0 else v


def _route_sources(i, d):
    return [_res(i, int(t)) for t in d["layers"].split(",")]


# users[i]: sections that read section i's output; shp[i]: its (C, H, W); concat[r] = (padded channels of route r's buffer,
# [(source, channel offset, padded width)] in `layers=` order); dest[s] = (r, offset): producer s writes straight into that slice
Layout = namedtuple("Layout", "users shp concat dest")


def analyse(defs, mods, cin, H, W):
    """Pure host function of the cfg: nothing is allocated and no library call is made."""
    users = [[] for _ in defs]
    for i, d in enumerate(defs):
        k = d["type"]
        if k in ("convolutional", "upsample", "maxpool", "yolo") and i > 0:
            users[i - 1].append(i)
        elif k == "route":
            for s in _route_sources(i, d):
                users[s].append(i)
        elif k == "shortcut":
            users[i - 1].append(i)
            users[_res(i, int(d["from"]))].append(i)
    shp = []
    c, h, w = cin, H, W
    for i, d in enumerate(defs):
        k = d["type"]
        if k == "convolutional":
            conv = mods[i][0]
            c = conv.out_channels
            h = (h + 2 * conv.padding[0] - conv.kernel_size[0]) // conv.stride[0] + 1
            w = (w + 2 * conv.padding[1] - conv.kernel_size[1]) // conv.stride[1] + 1
        elif k == "upsample":
            h, w = h * int(d["stride"]), w * int(d["stride"])
        elif k == "maxpool":
            ks, st = int(d["size"]), int(d["stride"])
            if not (ks == 2 and st == 1):                # (ZeroPad2d((0,1,0,1)) + MaxPool2d(2, 1) keeps the size, models.py:77-79)
                if ks > 15:
                    raise NotImplementedError("max-pool windows up to 15x15 are lowered")
                pp = (ks - 1) // 2                       # MaxPool2d(size, stride, (size - 1) // 2)
                h, w = (h + 2 * pp - ks) // st + 1, (w + 2 * pp - ks) // st + 1
        elif k == "route":
            src = _route_sources(i, d)
            c = sum(shp[s][0] for s in src)
            h, w = shp[src[0]][1], shp[src[0]][2]
        elif k == "shortcut":
            c, h, w = shp[i - 1]
        shp.append((c, h, w))
    concat, dest = {}, {}
    for i, d in enumerate(defs):
        src = _route_sources(i, d) if d["type"] == "route" else []
        if len(src) < 2:
            continue
        for s in src[:-1]:
            if shp[s][0] % 8:
                # the concat buffer places every source at a multiple-of-8 channel offset (16-byte vectors); the consumer's
                # packed weights index input channels contiguously, so a pad hole in the middle would misalign them
                raise NotImplementedError(f"[route] at section {i}: source {s} has {shp[s][0]} channels; every concat source but the "
                                          f"last must have a multiple of 8 channels")
        parts, off = [], 0
        for s in src:
            if s not in dest and defs[s]["type"] in ("convolutional", "upsample", "shortcut", "maxpool"):
                dest[s] = (i, off)
            parts.append((s, off, pad8(shp[s][0])))
            off += pad8(shp[s][0])
        concat[i] = (off, parts)
    return Layout(users, shp, concat, dest)


class Lowering:
    """What the forward lowerings of one plan share: the plan, the layout, the nodes made so far (`outs`, `cur`)."""

    def __init__(self, plan, net, layout, xin, B, T, with_targets):
        self.plan, self.layout, self.B, self.T, self.with_targets = plan, layout, B, T, with_targets
        self.defs, self.mods = net.module_defs, net.module_list
        self.slope = float(net.hyperparams["leaky_slope"])
        self.act_code = ACT_LEAKY if net.conv_activation == "leaky" else (ACT_RELU if net.conv_activation == "ReLU" else ACT_NONE)
        self.parents = {r: plan.new_act(B, layout.shp[r][1], layout.shp[r][2], ctot) for r, (ctot, _) in layout.concat.items()}
        self.outs = [None] * len(self.defs)
        self.cur = xin
        self.fused_into = {}                                 # shortcut section -> node of the conv that took it into its BatchNorm apply
        self.nbt = []                                        # num_batches_tracked of every BatchNorm with batch statistics
        self.rows_total = sum(self.mods[i][0].num_anchors * layout.shp[i][1] * layout.shp[i][2]
                              for i, d in enumerate(self.defs) if d["type"] == "yolo")
        self.row_off = 0

    def out_act(self, i):
        """the buffer section i writes: its slice of a concat buffer, or its own"""
        c, h, w = self.layout.shp[i]
        if i in self.layout.dest:
            r, off = self.layout.dest[i]
            return self.parents[r].slice(off, pad8(c))
        return self.plan.new_act(self.B, h, w, c)

    def done(self, i, node):
        self.outs[i] = self.cur = node


def lower_convolutional(cx, i, d):
    conv = cx.mods[i][0]
    if d["filters"] != "preyolo":
        return _lower_conv_bn(cx, i, conv, cx.mods[i][1])
    plan, x = cx.plan, cx.cur
    cs = ConvSpec(plan, conv.weight, conv.bias, conv.stride[0], conv.padding[0], 1, cin_pad=x.act.C)
    plan.emit_pack(cs, need_dgrad=cx.with_targets and x.needs_grad)
    y = TNode(cx.out_act(i), name="logits%d" % i)
    plan.emit_conv_fwd(cs, x.act, y.act)
    cx.done(i, y)
    return ConvLinear(cs, x, y)


@dataclass
class ConvLinear:
    """head conv: bias, no BatchNorm, no activation"""
    cs: ConvSpec
    x: TNode
    y: TNode

    def backward(self, plan):
        if self.y.gstate == "none":
            return
        plan.emit_bias_grad(self.cs, self.y.grad)
        plan.emit_conv_bwd(self.cs, self.x, self.y.act, self.y.grad)


def _lower_conv_bn(cx, i, conv, bn):
    """conv -> BatchNorm -> activation (-> + shortcut).  Four decisions, one emission sequence:
    pw_lb       a 1x1 conv right behind a BatchNorm-apply takes that pass into its operand load (engine.emit_pw_fwd)
    fuse        the [shortcut] behind this conv is its only user: the add rides in the BatchNorm apply, which writes the shortcut's output
    first2      the HBM-bound first conv (25 GFLOP, 88 MB in, 354 MB out at 416^2 x 32): statistics from one streaming pass over x, then
                y AND z = act(BatchNorm(y)) from a second one -- the layer's output is never re-read (csrc/first_conv.hip)
    one_launch  inference: BatchNorm + activation in the conv's store path"""
    plan, L, x, defs, B = cx.plan, cx.plan.L, cx.cur, cx.defs, cx.B
    bn_train, act_code, slope = plan.training, cx.act_code, cx.slope
    pw_lb = None
    if bn_train:                                             # decided before emit_pack so that the layer mark points at the fused launch
        pw_lb = plan.pw_fwd_candidate((conv.out_channels, conv.in_channels, conv.kernel_size[0], conv.kernel_size[1],
                                       conv.stride[0], conv.padding[0]), x.act)
        if pw_lb is not None:
            plan.fwd.pop()                                   # that bn_act_fwd entry is replaced by the fused launch below
    cs = ConvSpec(plan, conv.weight, conv.bias, conv.stride[0], conv.padding[0], 1, cin_pad=x.act.C)
    plan.emit_pack(cs, need_dgrad=cx.with_targets and x.needs_grad)
    ho, wo = cx.layout.shp[i][1], cx.layout.shp[i][2]
    bs = BnSpec(plan, bn)
    y = plan.new_act(B, ho, wo, conv.out_channels)
    fuse = (i + 1 < len(defs) and defs[i + 1]["type"] == "shortcut" and cx.layout.users[i] == [i + 1]
            and _res(i + 1, int(defs[i + 1]["from"])) != i)
    first2 = (bn_train and pw_lb is None and not fuse and plan.first_conv_2pass and cs.bias is None and plan.dtype == _lib.BF16 and
              bool(L.first_conv_ok(plan.cdt, B, x.act.H, x.act.W, cs.cin_pad, cs.cout_pad, cs.kh, cs.kw, cs.stride, cs.pad, cs.dil, x.act.ldc)))
    one_launch = not bn_train and netplan._EVAL_FUSE and not cx.with_targets
    # ---- the conv and the BatchNorm coefficients
    fold = None
    if bn_train:
        if first2:
            rows = int(L.first_conv_rows(B, ho))
            partial = plan.f32(rows * 2 * y.C, zero=False)
            plan.call(plan.fwd, L.first_conv_stats, plan.cdt, x.act.ptr, x.act.ldc, cs.wf.data_ptr(), partial.data_ptr(), B, x.act.H, x.act.W)
        elif pw_lb is not None:
            rows = int(L.pw_rows(x.act.M, cs.cin_pad))
            partial = plan.f32(rows * 2 * y.C, zero=False)
            plan.emit_pw_fwd(pw_lb, cs, x.act, y, partial)
        else:
            rows = plan.stats_rows(cs, x.act, y)
            partial = plan.f32(rows * 2 * y.C, zero=False)
            plan.emit_conv_fwd(cs, x.act, y, partial)
        conv_entry = plan.fwd[-1]
        plan.emit_bn_stats(bs, y, partial, rows)
        if not first2:
            fold = (conv_entry, plan.fwd[-1], cs, x.act, y, bs, partial, rows)
        cx.nbt.append(bn.num_batches_tracked)
    elif not one_launch:
        plan.emit_conv_fwd(cs, x.act, y)
        plan.emit_bn_eval(bs)
    # ---- apply + activation (+ shortcut) into the output node
    rnode = cx.outs[_res(i + 1, int(defs[i + 1]["from"]))] if fuse else None
    resid = rnode.act if fuse else None
    z = TNode(cx.out_act(i + 1), name="short%d" % (i + 1)) if fuse else TNode(cx.out_act(i), name="conv%d" % i)
    if first2:
        plan.call(plan.fwd, L.first_conv_bn_act, plan.cdt, x.act.ptr, x.act.ldc, cs.wf.data_ptr(), bs.scale.data_ptr(), bs.shift.data_ptr(),
                  act_code, slope, y.ptr, y.ldc, z.act.ptr, z.act.ldc, B, x.act.H, x.act.W)
        plan.last_bnact = None
        plan.first_conv_fwd2 = True
    elif one_launch:
        plan.emit_conv_bn_act_eval(cs, bs, x.act, z.act, act_code, slope, resid=resid)
    else:
        plan.emit_bn_act_fwd(y, bs, z.act, act_code, slope, resid=resid)
        if fold:
            plan.note_stats_fold(fold[0], fold[1], plan.fwd[-1], *fold[2:], z.act, act_code, slope, resid)
    cx.cur = z
    if fuse:
        cx.fused_into[i + 1] = z                             # (outs[i] stays None: nobody else reads it, `users[i] == [i + 1]`)
    else:
        cx.outs[i] = z
    return ConvBn(cs, bs, x, y, z, rnode, act_code, slope)


@dataclass
class ConvBn:
    cs: ConvSpec
    bs: BnSpec
    x: TNode
    y: Act                      # raw conv output
    z: TNode                    # act(BatchNorm(y)) (+ resid)
    resid: TNode                # the other operand of a shortcut taken into the apply, or None
    act_code: int
    slope: float

    def backward(self, plan):
        if self.z.gstate == "none":
            return
        if self.resid is not None:
            plan.grad_identity(self.resid, self.z.grad)
        if not plan.emit_first_conv_bwd(self.z.grad, self.y, self.bs, self.act_code, self.slope, self.cs, self.x):
            dy = plan.emit_bn_act_bwd(self.z.grad, self.y, self.bs, self.act_code, self.slope)
            plan.emit_conv_bwd(self.cs, self.x, self.y, dy)


def lower_shortcut(cx, i, d):
    if i in cx.fused_into:
        cx.done(i, cx.fused_into[i])
        return None
    a, b = cx.outs[i - 1], cx.outs[_res(i, int(d["from"]))]
    z = TNode(cx.out_act(i), name="short%d" % i)
    cx.plan.emit_add(cx.plan.fwd, a.act, b.act, z.act)
    cx.done(i, z)
    return Shortcut(a, b, z)


@dataclass
class Shortcut:
    a: TNode
    b: TNode
    z: TNode

    def backward(self, plan):
        if self.z.gstate == "none":
            return
        plan.grad_identity(self.a, self.z.grad)
        plan.grad_identity(self.b, self.z.grad)


def lower_maxpool(cx, i, d):
    plan, L, x = cx.plan, cx.plan.L, cx.cur
    ks, st = int(d["size"]), int(d["stride"])
    z = TNode(cx.out_act(i), name="pool%d" % i)
    a = x.act
    idx = torch.empty(z.act.M * z.act.C, dtype=torch.uint8, device=plan.device)
    plan.keep.append(idx)
    two = ks == 2 and st in (1, 2)                           # the pools of yolo_baseline_tiny.cfg
    if two:
        plan.call(plan.fwd, L.maxpool2x2_fwd, plan.dtype, a.ptr, a.ldc, z.act.ptr, z.act.ldc, idx.data_ptr(), cx.B, a.H, a.W, a.C, st)
    else:
        plan.call(plan.fwd, L.maxpool_fwd, plan.dtype, a.ptr, a.ldc, z.act.ptr, z.act.ldc, idx.data_ptr(), cx.B, a.H, a.W, a.C, ks, st, (ks - 1) // 2)
    cx.done(i, z)
    return MaxPool(x, z, idx, ks, st, two)


@dataclass
class MaxPool:
    x: TNode
    z: TNode
    idx: torch.Tensor           # arg-max position per output element
    ks: int
    stride: int
    two: bool                   # the 2x2 kernel pair (maxpool2x2_*) instead of the general one

    def backward(self, plan):
        if self.z.gstate == "none":
            return
        L, xa, g = plan.L, self.x.act, self.z.grad
        out, add = plan.grad_target(self.x)
        tgt = out if add is None else plan.new_act(xa.B, xa.H, xa.W, xa.C)
        if self.two:
            plan.call(plan.bwd, L.maxpool2x2_bwd, plan.dtype, g.ptr, g.ldc, self.idx.data_ptr(), tgt.ptr, tgt.ldc, xa.B, xa.H, xa.W, xa.C, self.stride)
        else:
            plan.call(plan.bwd, L.maxpool_bwd, plan.dtype, g.ptr, g.ldc, self.idx.data_ptr(), tgt.ptr, tgt.ldc, xa.B, xa.H, xa.W, xa.C,
                      self.ks, self.stride, (self.ks - 1) // 2)
        if add is not None:
            plan.emit_add(plan.bwd, tgt, add, out)


def lower_upsample(cx, i, d):
    plan, L, x = cx.plan, cx.plan.L, cx.cur
    sc = int(d["stride"])
    z = TNode(cx.out_act(i), name="up%d" % i)
    a = x.act
    if sc == 2:
        plan.call(plan.fwd, L.upsample2x_fwd, plan.dtype, a.ptr, a.ldc, z.act.ptr, z.act.ldc, cx.B, a.H, a.W, a.C)
    else:
        plan.call(plan.fwd, L.upsample_fwd, plan.dtype, a.ptr, a.ldc, z.act.ptr, z.act.ldc, cx.B, a.H, a.W, a.C, sc)
    cx.done(i, z)
    return Upsample(x, z, sc)


@dataclass
class Upsample:
    x: TNode
    z: TNode
    scale: int

    def backward(self, plan):
        if self.z.gstate == "none":
            return
        L, xa, g = plan.L, self.x.act, self.z.grad
        out, add = plan.grad_target(self.x)
        fn, extra = (L.upsample2x_bwd, ()) if self.scale == 2 else (L.upsample_bwd, (self.scale,))
        tgt = out if add is None else plan.new_act(xa.B, xa.H, xa.W, xa.C)
        plan.call(plan.bwd, fn, plan.dtype, g.ptr, g.ldc, tgt.ptr, tgt.ldc, xa.B, xa.H, xa.W, xa.C, *extra)
        if add is not None:
            plan.emit_add(plan.bwd, tgt, add, out)


def lower_route(cx, i, d):
    src = _route_sources(i, d)
    if len(src) == 1:
        cx.done(i, cx.outs[src[0]])
        return None
    plan, par = cx.plan, cx.parents[i]
    z = TNode(par, name="route%d" % i)
    off = 0
    parts = []
    for s in src:
        sn = cx.outs[s]
        sl = par.slice(off, sn.act.C)
        inplace = cx.layout.dest.get(s, (None,))[0] == i and sn.act.ptr == sl.ptr
        if not inplace:                                      # fallback: explicit copy into the slice
            plan.emit_add(plan.fwd, sn.act, None, sl)
        parts.append((sn, off))
        off += sn.act.C
    cx.done(i, z)
    return Concat(parts, z)


@dataclass
class Concat:
    parts: list                 # (source TNode, channel offset in z)
    z: TNode

    def backward(self, plan):
        if self.z.gstate == "none":
            return
        for sn, off in self.parts:
            plan.grad_identity(sn, self.z.grad.slice(off, sn.act.C))


def lower_yolo(cx, i, d):
    plan, L, lg, B = cx.plan, cx.plan.L, cx.cur, cx.B
    yl = cx.mods[i][0]
    Gh, Gw = lg.act.H, lg.act.W
    anchors = yl.scaled_anchors(Gh).to(plan.device)
    plan.keep.append(anchors)
    A, C = yl.num_anchors, yl.num_classes
    cx.outs[i] = lg
    if not cx.with_targets:
        plan.call(plan.fwd, L.yolo_head_decode, plan.dtype, lg.act.ptr, lg.act.ldc, anchors.data_ptr(), float(yl.stride_for(Gh)), B, A, C,
                  Gh, Gw, plan.eval_out.data_ptr(), cx.rows_total, cx.row_off)
        cx.row_off += A * Gh * Gw
        return None
    ws = torch.zeros(int(L.yolo_head_workspace_bytes(B, A, Gh, Gw)), dtype=torch.uint8, device=plan.device)
    plan.keep.append(ws)
    geo = (B, cx.T, A, C, Gh, Gw, float(yl.ignore_thres), float(yl.xy_loss), float(yl.wh_loss), float(yl.object_loss), float(yl.no_object_loss))
    plan.call(plan.fwd, L.yolo_head_train, plan.dtype, lg.act.ptr, lg.act.ldc, None, 0, lg.act.C, plan.targets.data_ptr(),
              anchors.data_ptr(), *geo, ws.data_ptr(), plan.out7.data_ptr(), None)
    plan.watch_head(ws, B, A, Gh, Gw)
    return YoloHead(lg, anchors, ws, geo)


@dataclass
class YoloHead:
    lg: TNode                   # logits
    anchors: torch.Tensor
    ws: torch.Tensor            # head workspace (csrc/yolo_head.hip)
    geo: tuple

    def backward(self, plan):
        lg = self.lg
        out, add = plan.grad_target(lg)
        assert add is None
        plan.call(plan.bwd, plan.L.yolo_head_grad, plan.dtype, lg.act.ptr, lg.act.ldc, out.ptr, out.ldc, out.C, plan.targets.data_ptr(),
                  self.anchors.data_ptr(), *self.geo, self.ws.data_ptr(), plan.gscale.data_ptr())


FORWARD = {"convolutional": lower_convolutional, "shortcut": lower_shortcut, "maxpool": lower_maxpool, "upsample": lower_upsample,
           "route": lower_route, "yolo": lower_yolo}
