"""The plan audit (tests/helpers/plan_audit.py: method, bounds) for KeypointNet's records: the 7x7 stem, the residual blocks -- dilated conv1 ->
BatchNorm -> ReLU, then relu(bn2(conv2(mid)) + shortcut_bn(shortcut_conv(x))) in ONE apply launch --, the head conv and the soft-argmax head.

A block is two units: "conv1" (x -> mid) and "sum" (mid, x -> out), the latter with two conv -> BatchNorm branches under one activation; the
bounds are plan_audit's per branch, with the pre-activation's error the sum of the branches' (one kink test for both).  Every conv has a bias in
front of its BatchNorm: it enters y and the statistics, its gradient is exactly zero and must be stored as zero.  In bf16 plans the head conv
writes float32 logits from the MASTER weights (csrc/rektnet_head.hip), its data gradient uses the packed bf16 weights.  The loss lives outside the
plan: the plan's outputs are (hm, pts) and its output gradient is the device's dpts.
"""
import torch
import torch.nn.functional as F

import head_refs as hr
import plan_audit as pa
from plan_audit import U, D, acc, _conv, _stat_bounds, _stat_gap, conv_backward, Unit

from oracle import rektnet_oracle as ro

EPS = 1e-5


def c4(v):
    return v.view(1, -1, 1, 1)


def geometry():
    """conv name -> dict(stride, pad, dil)"""
    return {name: dict(stride=1, pad=pad, dil=dil) for name, _, _, _, pad, dil in ro.conv_specs()}


def units():
    """[(Unit, [(conv, bn, source node)])]: nodes are "in", "a0".."a4" (block outputs) and "m1".."m4" (mid)"""
    out = [(Unit("stem", "ConvBn", ["in"], "a0", {}), [("conv", "bn", "in")])]
    for r in range(1, 5):
        x, mid, o = f"a{r - 1}", f"m{r}", f"a{r}"
        out.append((Unit(f"res{r}.conv1", "ConvBn", [x], mid, {}), [(f"res{r}.conv1", f"res{r}.bn1", x)]))
        out.append((Unit(f"res{r}.sum", "DualBn", [mid, x], o, {}),
                    [(f"res{r}.conv2", f"res{r}.bn2", mid), (f"res{r}.shortcut_conv", f"res{r}.shortcut_bn", x)]))
    return out


def branches_forward(P, br, running=None):
    """br: [dict(x, w, b, gamma, beta, L)] -> per branch (y, e_y, mean, e_mean, invstd, e_invstd), and (z, e_z) of relu(sum of the branches)"""
    per, t, e_t = [], 0.0, 0.0
    for k, b in enumerate(br):
        y = _conv(b["x"], b["w"], b["L"], b["b"])
        K = b["w"].shape[1] * b["w"].shape[2] * b["w"].shape[3]
        e_acc = acc(K) * (_conv(b["x"].abs(), b["w"].abs(), b["L"]) + c4(b["b"].abs()))
        e_y = e_acc + P.rnd(y.abs() + e_acc)
        if running is None:
            mean, var, inv, e_mean, e_inv = _stat_bounds(y, e_acc, EPS)
        else:
            mean, var = running[k]
            inv = (var + EPS).rsqrt()
            e_mean, e_inv = torch.zeros_like(mean), 4 * U * inv
        tk = c4(b["gamma"]) * (y - c4(mean)) * c4(inv) + c4(b["beta"])
        e_t = e_t + (c4(b["gamma"].abs()) * (c4(inv) * (e_y + c4(e_mean)) + (y - c4(mean)).abs() * c4(e_inv))
                     + 8 * U * (tk.abs() + c4(b["beta"].abs()) + c4((b["gamma"] * mean * inv).abs())))
        t = t + tk
        per.append((y, e_y, mean, e_mean, inv, e_inv))
    z = F.relu(t)
    if len(br) > 1:
        e_t = e_t + 2 * U * t.abs()
    return per, (z, e_t + P.rnd(z.abs() + e_t))


def branches_backward(P, br, ys, dz, need_dx, stats=None):
    """br as above, ys: the device's raw conv outputs -> per branch dict(dW, dgamma, dbeta, dx) of (expected, bound)"""
    leaves = []
    t = 0.0
    for b, y in zip(br, ys):
        yl, gl, bl = y.clone().requires_grad_(True), b["gamma"].clone().requires_grad_(True), b["beta"].clone().requires_grad_(True)
        mean, var = yl.mean((0, 2, 3)), yl.var((0, 2, 3), unbiased=False)
        inv = (var + EPS).rsqrt()
        xhat = (yl - c4(mean)) * c4(inv)
        t = t + c4(gl) * xhat + c4(bl)
        leaves.append((yl, gl, bl, mean.detach(), inv.detach(), xhat.detach()))
    z = F.relu(t)
    grads = torch.autograd.grad(z, [v for lf in leaves for v in lf[:3]], dz)
    t = t.detach()
    K = dz.numel() // dz.shape[1]
    e_t, ex = 0.0, []
    for k, (b, y, lf) in enumerate(zip(br, ys, leaves)):
        _, _, _, mean, inv, xhat = lf
        d_mean, d_inv = _stat_gap(P, y, mean, inv, stats[k] if stats is not None else None, EPS)
        e_xhat = c4(inv) * c4(d_mean) + (y - c4(mean)).abs() * c4(d_inv) + 4 * U * xhat.abs()
        ex.append((e_xhat, d_inv))
        e_t = e_t + c4(b["gamma"].abs()) * e_xhat + 8 * U * ((c4(b["gamma"]) * xhat).abs() + c4(b["beta"].abs()))
    kink = t.abs() <= e_t
    g = dz * (t > 0).to(D)
    e_g = torch.where(kink, dz.abs(), 4 * U * g.abs())
    out = []
    for k, (b, y, lf) in enumerate(zip(br, ys, leaves)):
        _, _, _, mean, inv, xhat = lf
        dy, dgamma, dbeta = grads[3 * k:3 * k + 3]
        e_xhat, d_inv = ex[k]
        dims = (0, 2, 3)
        e_dbeta = e_g.sum(dims) + acc(K) * g.abs().sum(dims)
        e_dgamma = ((e_g * xhat.abs() + g.abs() * e_xhat).sum(dims) + acc(K) * inv * ((g * y).abs().sum(dims) + mean.abs() * g.abs().sum(dims)))
        gi = c4(b["gamma"].abs() * inv)
        e_dy = (gi * (e_g + c4(e_dbeta) / K + e_xhat * c4(dgamma.abs()) / K + xhat.abs() * c4(e_dgamma) / K) + dy.abs() * c4(d_inv / inv)
                + 8 * U * gi * (g.abs() + c4(dbeta.abs()) / K + c4(dgamma.abs()) / K * c4(inv) * (y.abs() + c4(mean.abs()))))
        e_dy = e_dy + P.rnd(dy.abs() + e_dy)
        r = {"dgamma": (dgamma, e_dgamma), "dbeta": (dbeta, e_dbeta)}
        r.update(conv_backward(b["x"], b["w"], dy, e_dy, b["L"], need_dx[k]))
        out.append(r)
    return out


class KTensors:
    def __init__(self):
        self.act, self.grad, self.y, self.mean, self.invstd, self.pgrad = {}, {}, {}, {}, {}, {}
        self.lg = self.hm = self.pts = self.dpts = self.dlg = None


def audit_keypoint(P, sd, tens, report, train=True):
    """sd: float64 state dict (masters, running statistics for eval plans).  tens: KTensors read from the plan (or an emulation)."""
    geo = geometry()
    contribs = {}
    for u, convs in units():
        br = [dict(x=tens.act[src], w=P.weights(sd[f"{cv}.weight"]), b=sd[f"{cv}.bias"], gamma=sd[f"{bn}.weight"], beta=sd[f"{bn}.bias"],
                   L=geo[cv]) for cv, bn, src in convs]
        running = None if train else [(sd[f"{bn}.running_mean"], sd[f"{bn}.running_var"]) for _, bn, _ in convs]
        per, (z, e_z) = branches_forward(P, br, running)
        for (cv, bn, _), (y, e_y, mean, e_mean, inv, e_inv) in zip(convs, per):
            if cv in tens.y:
                report.check(u, f"y({cv})", tens.y[cv], y, e_y)
            if train:
                report.check(u, f"mean({bn})", tens.mean[bn], mean, e_mean)
                report.check(u, f"invstd({bn})", tens.invstd[bn], inv, e_inv)
        report.check(u, "z", tens.act[u.out], z, e_z)
        if not train:
            continue
        need = [src != "in" for _, _, src in convs]
        back = branches_backward(P, br, [tens.y[cv] for cv, _, _ in convs], tens.grad[u.out], need,
                                 stats=[(tens.mean[bn], tens.invstd[bn]) for _, bn, _ in convs])
        for (cv, bn, src), r in zip(convs, back):
            report.check(u, f"dW({cv})", tens.pgrad[f"{cv}.weight"], *r["dW"])
            report.check(u, f"dgamma({bn})", tens.pgrad[f"{bn}.weight"], *r["dgamma"])
            report.check(u, f"dbeta({bn})", tens.pgrad[f"{bn}.bias"], *r["dbeta"])
            report.check(u, f"dbias({cv})", tens.pgrad[f"{cv}.bias"], torch.zeros_like(sd[f"{cv}.bias"]), 0.0)
            if src != "in":
                contribs.setdefault(src, []).append((u, r["dx"][0], r["dx"][1], True))
    # ---- head conv (float32 logits from the master weights in bf16 plans) and soft-argmax
    uh, us = Unit("out", "ConvLinear", ["a4"], "lg", {}), Unit("softargmax", "SoftArgmax", ["lg"], None, {})
    L = geo["out"]
    x, w, b = tens.act["a4"], sd["out.weight"], sd["out.bias"]
    y = _conv(x, w, L, b)
    e_y = acc(w.shape[1]) * (_conv(x.abs(), w.abs(), L) + c4(b.abs()))
    report.check(uh, "y", tens.lg, y, e_y + U * (y.abs() + e_y))
    hm64, pt64 = hr.softargmax(tens.lg, D)
    hm32, pt32 = hr.softargmax(tens.lg, torch.float32)
    report.check(us, "hm", tens.hm, hm64, hr.bound(hr.maxabs(hm32.double() - hm64), hr.maxabs(hm64)))
    report.check(us, "pts", tens.pts, pt64, hr.bound(hr.maxabs(pt32.double() - pt64), hr.maxabs(pt64)))
    if train:
        g64 = hr.softargmax_bwd(tens.lg, tens.dpts, None, D)
        g32 = hr.softargmax_bwd(tens.lg, tens.dpts, None, torch.float32)
        e = torch.full_like(g64, hr.bound(hr.maxabs(g32 - g64), hr.maxabs(g64)))
        report.check(us, "dlogits", tens.dlg, g64, e + P.rnd(g64.abs() + e))
        r = conv_backward(x, P.weights(w), tens.dlg, None, L, True)
        report.check(uh, "dW", tens.pgrad["out.weight"], *r["dW"])
        Kb = tens.dlg.numel() // tens.dlg.shape[1]
        report.check(uh, "dbias", tens.pgrad["out.bias"], tens.dlg.sum((0, 2, 3)), acc(Kb) * tens.dlg.abs().sum((0, 2, 3)))
        contribs.setdefault("a4", []).append((uh, r["dx"][0], r["dx"][1], True))
        for node, cl in contribs.items():
            want, bnd = pa.node_grad(P, [(v, bd, comp) for _, v, bd, comp in cl])
            report.check([cc[0] for cc in cl], f"grad of node {node}", tens.grad[node], want, bnd)


# ------------------------------------------------------------------------------------------------ host: exact decomposition and emulation
def run_keypoint(P, sd, x, dpts_fn, emulate):
    """The units on their own outputs.  emulate=False: float64, exact (-> decomposition against the oracle's autograd); emulate=True: float32
    arithmetic with P's stores at y, z, dy, the gradient contributions and their accumulations.  dpts_fn(pts) -> the plan's output gradient."""
    dt = torch.float32 if emulate else D
    st = P.store if emulate else (lambda v: v)
    geo = geometry()
    T = KTensors()
    W = {k: (st(v.to(dt)) if (emulate and k.endswith("weight") and v.dim() == 4) else v.to(dt)) for k, v in sd.items()}
    T.act["in"] = st(x.to(dt))
    for u, convs in units():
        t = 0.0
        for cv, bn, src in convs:
            y = _conv(T.act[src], W[f"{cv}.weight"], geo[cv], W[f"{cv}.bias"])
            mean = y.mean((0, 2, 3))
            var = ((y * y).mean((0, 2, 3)).double() - mean.double() ** 2).to(dt) if emulate else y.var((0, 2, 3), unbiased=False)
            inv = (var + EPS).rsqrt()
            T.y[cv], T.mean[bn], T.invstd[bn] = st(y), mean, inv
            scale = W[f"{bn}.weight"] * inv
            t = t + T.y[cv] * c4(scale) + c4(W[f"{bn}.bias"] - mean * scale)
        T.act[u.out] = st(F.relu(t))
    wh = sd["out.weight"].to(dt)                                   # the head's forward reads the masters
    T.lg = _conv(T.act["a4"], wh, geo["out"], W["out.bias"])
    T.hm, T.pts = hr.softargmax(T.lg, dt)
    T.dpts = dpts_fn(T.pts).to(dt)
    T.dlg = st(hr.softargmax_bwd(T.lg, T.dpts, None, dt).to(dt))

    def add(node, v):
        v = st(v)
        T.grad[node] = v if node not in T.grad else st(T.grad[node] + v)

    def conv_grads(xx, ww, L, dy):
        xx, ww = xx.clone().requires_grad_(True), ww.clone().requires_grad_(True)
        return torch.autograd.grad(_conv(xx, ww, L), [xx, ww], dy)
    dx, dw = conv_grads(T.act["a4"], W["out.weight"], geo["out"], T.dlg)
    T.pgrad["out.weight"], T.pgrad["out.bias"] = dw, T.dlg.sum((0, 2, 3))
    add("a4", dx)
    for u, convs in reversed(units()):
        dz = T.grad[u.out]
        leaves, t = [], 0.0
        for cv, bn, src in convs:
            yl = T.y[cv].clone().requires_grad_(True)
            gl, bl = W[f"{bn}.weight"].clone().requires_grad_(True), W[f"{bn}.bias"].clone().requires_grad_(True)
            if emulate:                                            # the device's own statistics as constants, dy from the closed form below
                xhat = (yl - c4(T.mean[bn])) * c4(T.invstd[bn])
            else:
                xhat = (yl - c4(yl.mean((0, 2, 3)))) * c4((yl.var((0, 2, 3), unbiased=False) + EPS).rsqrt())
            t = t + c4(gl) * xhat + c4(bl)
            leaves.append((yl, gl, bl, xhat.detach()))
        if emulate:
            g = dz * (t.detach() > 0).to(dt)
            K = dz.numel() // dz.shape[1]
        else:
            grads = torch.autograd.grad(F.relu(t), [v for lf in leaves for v in lf[:3]], dz)
        for k, ((cv, bn, src), lf) in enumerate(zip(convs, leaves)):
            if emulate:
                xhat = lf[3]
                dbeta, dgamma = g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))
                dy = st(c4(W[f"{bn}.weight"] * T.invstd[bn]) * (g - c4(dbeta) / K - xhat * c4(dgamma) / K))
            else:
                dy, dgamma, dbeta = grads[3 * k:3 * k + 3]
            dx, dw = conv_grads(T.act[src], W[f"{cv}.weight"], geo[cv], dy)
            T.pgrad[f"{cv}.weight"], T.pgrad[f"{bn}.weight"], T.pgrad[f"{bn}.bias"] = dw, dgamma, dbeta
            T.pgrad[f"{cv}.bias"] = torch.zeros_like(W[f"{cv}.bias"])
            if src != "in":
                add(src, dx)
    for name in ("act", "grad", "y", "mean", "invstd", "pgrad"):
        setattr(T, name, {k: v.to(D) for k, v in getattr(T, name).items()})
    T.lg, T.hm, T.pts, T.dpts, T.dlg = (v.to(D) for v in (T.lg, T.hm, T.pts, T.dpts, T.dlg))
    return T


def keypoint_state(seed):
    """float64 state dict: rektnet_oracle.init_state with non-zero biases, a non-trivial BatchNorm affine and running statistics"""
    sd = ro.init_state(seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k, v in sd.items():
        if k.endswith("running_var"):
            sd[k] = torch.rand(v.shape, generator=g) * 1.5 + 0.5
        elif k.endswith("running_mean"):
            sd[k] = (torch.rand(v.shape, generator=g) - 0.5) * 0.4
        elif v.dim() == 1 and ("bn" in k) and k.endswith("weight"):
            sd[k] = torch.rand(v.shape, generator=g) * 0.5 + 0.75
        elif v.dim() == 1:
            sd[k] = (torch.rand(v.shape, generator=g) - 0.5) * 0.2
    return {k: v.to(D) for k, v in sd.items()}


def keypoint_batch():
    g = torch.Generator().manual_seed(9)
    return torch.rand(4, 3, 80, 80, generator=g), torch.rand(4, 7, 2, generator=g) * (79 / 80)


def loss_grad(tpts):
    """pts -> d(total cross-ratio loss)/d pts in float64 (the loss is outside the plan; any smooth function of pts would do)"""
    def fn(pts):
        p = pts.detach().to(D).clone().requires_grad_(True)
        ro.cross_ratio_loss(None, p, None, tpts.to(D), "l1_softargmax", True, 0.05, 0.05)[2].backward()
        return p.grad
    return fn
