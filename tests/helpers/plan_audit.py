"""Teacher-forced float64 reference of a launch plan, unit by unit, with derived per-element bounds (tests/test_plan_audit_host.py,
tests/test_gpu_plan_audit.py).

A plan is audited from its own tensors: every unit of the lowering (one cfg section, or a conv with the shortcut folded into its BatchNorm
apply) is re-evaluated in float64 on the CPU from the tensors the device itself left one step upstream -- its inputs, the master weights
(rounded to bf16 round-to-nearest-even for bf16 plans, what the pack kernel is tested to do), its own raw conv output for the backward, its
own output gradient -- so no error is carried from layer to layer and a wiring mistake shows as an O(1) miss of ONE unit.  Which node feeds
which unit comes from `Graph`, an analysis of the cfg that shares no code with yolo/lower.py.  Gradients come from torch autograd on the
one-unit float64 graph; nothing here restates a kernel's formula except where a bound needs the magnitude of an intermediate.

The expected gradient of a node is the sum of its consumers' contributions, each from that consumer's device-side output gradient
(`node_grad`).

Bounds.  u = 2^-24.  "s (m)" is the bound of one store of a value of magnitude <= m: half a unit in the last place of bf16 at m
(head_refs.half_ulp_bf16; bf16 plans) or u m (fp32 plans: every bf16 store becomes one fp32 rounding).  Half a unit in the last place is
2^-9 |v| only at the top of a binade and 2^-8 |v| at its bottom (1.00390 is stored as 1.0: the emulation below meets error / (2^-9 |v|) = 1.99
on y), so 2^-9 |v| is not a bound of one store; the exact half-ulp is.  |.| is elementwise,
"acc(K) mag" = (K + 2) u mag where mag is the same operation on absolute values (any summation order of K terms in fp32).
  y      raw conv output: one store.                      acc(taps cin) conv(|x|,|w|) + s (|y| + that)
  mean   of the K = B H W values of a channel; the conv epilogues take the fp32 accumulators, not the stored y (csrc/conv_gemm.h, first_conv.hip),
         so each value carries e_a = acc(taps cin) conv(|x|,|w|) only:   mean(e_a) + acc(K) mean|y|
  var    E[y^2] - mean^2, cancellation written out:       e_q = mean(2|y| e_a + e_a^2) + acc(K) E[y^2];  e_var = e_q + 2|mean| e_mean + e_mean^2
         (the subtraction itself is done in float64 by the finalize kernels); relative to var this grows like mean^2 / var.
  invstd (var + eps)^-1/2 evaluated at var -+ e_var (exact interval, no linearisation) + 4 u invstd
  z      act is 1-Lipschitz, one store:                   e_t = |gamma| (invstd (e_y + e_mean) + |y - mean| e_invstd) + 8 u (|t| + |beta|);  e_t + s (|z| + e_t)
  backward of conv -> BatchNorm -> act, from (x, device y, dz).  The reference statistics are those of the device's y in float64; the device's own
  mean / invstd (inputs of its backward, audited by the forward) differ from them by d_mean, d_invstd, taken as they are (+ 4 u); e_xhat follows.
  g      dz act'(t): where |t| <= e_t' (t within its own error of the kink) the device may take the other slope: (1 - slope) |dz|, else 4 u |g|
  dbeta  sum e_g + acc(K) sum|g|
  dgamma sum(e_g |xhat| + |g| e_xhat) + acc(K) invstd (sum|g y| + |mean| sum|g|)       (the kernels may sum g y and g separately)
  dy     one store, named dy: |gamma| invstd (e_g + e_dbeta/K + e_xhat |dgamma|/K + |xhat| e_dgamma/K) + |dy| e_invstd/invstd
         + 8 u |gamma| invstd (|g| + |dbeta|/K + |dgamma|/K invstd (|y| + |mean|)) [dy = cA g + cB y + cC cancels in fp32] + s |dy|
  dW     wgrad(e_dy, |x|) + acc(B Ho Wo) wgrad(|dy|, |x|)     (intermediate propagation of dy's store through the one remaining linear op)
  dx     dgrad(e_dy, |w|) + acc(taps cout) dgrad(|dy|, |w|)   (its own store is counted at the node, below)
  head conv: the same with dy = the device's gradient of the logits (e_dy = 0); bias gradient acc(B H W) sum|dy|.
  node gradient with n consumers of which c are computed (conv data gradients, pool / upsample backward, YOLO head) and n - c are identities
  (shortcut branch, concat slice): an alias (n = 1, c = 0) is exact; otherwise at most c + (n - 1) stores (each computed contribution once, to the
  buffer or a temporary, and one per accumulation), each of a partial sum no larger than sum_k |contribution_k|:
         sum_k e_k + (c + n - 1) s sum_k(|contribution_k| + e_k)
  max-pool forward and upsample forward are exact; upsample backward sums scale^2 values: acc(scale^2); max-pool backward is exact where the
  windows do not overlap, sums up to k^2 window gradients where they do (size 2 stride 1: acc(k^2) of the same scatter of |dz|; the device met
  16 u |v| there under cancellation before this term was written down), and where a window's maximum is attained twice (bf16 values tie
  often) either position may take the gradient: bound |dz| of that window there.
  YOLO head: head_refs.bound(|f32 - f64|, scale) of the same torch expression, as tests/test_gpu_heads.py, + one store for the gradient.
  inference plans (running statistics, conv + BatchNorm + act in one launch): no statistics terms; with a folded shortcut the launch rounds
  act(t) and then the sum (see audit_darknet), two stores.
No bound is multiplied by a safety factor.

Largest error / bound per unit kind.  Host = the float32 / bf16-store emulation below against the float64 reference at the shapes of the GPU
test (tests/test_plan_audit_host.py prints them); device = MI355X, printed by tests/test_gpu_plan_audit.py.
(kind.tensor host/device; '-' = not measured there; the largest over the audit nets and the configurations of the tests)
A ratio of exactly 1 is a store that fell on a tie (error = half a unit in the last place, which the bound equals); the max-pool and upsample
backward show under node.grad.
  Darknet, inference, bf16
    Concat.z -/0  ConvBn.z -/0.994  ConvLinear.y -/0.998  MaxPool.z -/0  Shortcut.z -/1  Upsample.z -/0  YoloHead.rows -/0.0353
  Darknet, inference, fp32
    Concat.z -/0  ConvBn.z -/0.093  ConvLinear.y -/0.059  MaxPool.z -/0  Shortcut.z -/1  Upsample.z -/0  YoloHead.rows -/0.0389
  Darknet, training, bf16
    Concat.z 0/0  ConvBn.dW 0.968/0.959  ConvBn.dbeta 1/1  ConvBn.dgamma 0.999/0.997  ConvBn.invstd 0.0085/0.0107
    ConvBn.mean 0.0101/0.0116  ConvBn.y 0.999/0.999  ConvBn.z 0.965/0.981  ConvLinear.dW 0.0487/0.108  ConvLinear.dbias 0/0
    ConvLinear.y 0.998/0.995  MaxPool.z 0/0  Shortcut.z 1/1  Upsample.z 0/0  YoloHead.loss 0.0472/0.0266  YoloHead.parts 0.0671/0.0664
    node.grad 1/1
  Darknet, training, fp32
    Concat.z 0/0  ConvBn.dW 0.116/0.12  ConvBn.dbeta 0.0997/0.0616  ConvBn.dgamma 0.0781/0.0956  ConvBn.invstd 0.0156/0.0116
    ConvBn.mean 0.0283/0.026  ConvBn.y 0.142/0.142  ConvBn.z 0.0233/0.0363  ConvLinear.dW 0.0918/0.135  ConvLinear.dbias 0.0371/0.0713
    ConvLinear.y 0.077/0.0726  MaxPool.z 0/0  Shortcut.z 1/1  Upsample.z 0/0  YoloHead.loss 0.0635/0.0386  YoloHead.parts 0.125/0.0537
    node.grad 1/1
  KeypointNet, inference, bf16
    ConvBn.z -/0.987  ConvLinear.y -/0.0113  DualBn.y -/1  DualBn.z -/0.982  SoftArgmax.hm -/0.0637  SoftArgmax.pts -/0.0735
  KeypointNet, inference, fp32
    ConvBn.z -/0.0314  ConvLinear.y -/0.0169  DualBn.y -/0.189  DualBn.z -/0.035  SoftArgmax.hm -/0.0419  SoftArgmax.pts -/0.0826
  KeypointNet, training, bf16
    ConvBn.dW 0.13/0.136  ConvBn.dbeta 0.387/0.387  ConvBn.dbias 0/0  ConvBn.dgamma 0.0226/0.0227  ConvBn.invstd 0.0001/0.0001
    ConvBn.mean 0.0001/0  ConvBn.y 0.995/0.995  ConvBn.z 0.803/0.803  ConvLinear.dW 0.0006/0.0001  ConvLinear.dbias 0/0.0001
    ConvLinear.y 0.0292/0.0116  DualBn.dW 0.405/0.39  DualBn.dbeta 0.36/0.36  DualBn.dbias 0/0  DualBn.dgamma 0.219/0.218
    DualBn.invstd 0.0001/0.0001  DualBn.mean 0.0001/0.0001  DualBn.y 1/1  DualBn.z 0.732/0.732  SoftArgmax.dlogits 0.977/0.962
    SoftArgmax.hm 0.125/0.0249  SoftArgmax.pts 0.125/0.0196  node.grad 1/1
  KeypointNet, training, fp32
    ConvBn.dW 0.0002/0  ConvBn.dbeta 0/0  ConvBn.dbias 0/0  ConvBn.dgamma 0/0  ConvBn.invstd 0.0001/0  ConvBn.mean 0.0001/0
    ConvBn.y 0.0334/0.0349  ConvBn.z 0.0011/0.0011  ConvLinear.dW 0.0006/0.0002  ConvLinear.dbias 0/0.0001  ConvLinear.y 0.0359/0.0286
    DualBn.dW 0.0086/0.0001  DualBn.dbeta 0.0052/0  DualBn.dbias 0/0  DualBn.dgamma 0.0022/0  DualBn.invstd 0.0001/0.0001
    DualBn.mean 0.0001/0  DualBn.y 0.201/0.237  DualBn.z 0.0004/0.0006  SoftArgmax.dlogits 0.125/0.0669  SoftArgmax.hm 0.125/0.0242
    SoftArgmax.pts 0.125/0.0277  node.grad 0.516/0.534
"""
import math

import torch
import torch.nn.functional as F

from oracle import yolo_oracle as yo
import head_refs as hr

U = 2.0 ** -24
D = torch.float64


def rne_bf16(t):
    """float64 tensor of the values rounded to bf16, round-to-nearest-even (through float32, which is exact for float32 masters)"""
    return t.to(torch.float32).to(torch.bfloat16).to(D)


class Prec:
    def __init__(self, bf16):
        self.bf16 = bool(bf16)
        self.s = 2.0 ** -8 if bf16 else U

    def weights(self, w):
        return rne_bf16(w) if self.bf16 else w.to(D)

    def rnd(self, mag):
        """bound of the rounding of one store of a value of magnitude <= mag: half a unit in the last place of the plan's type there"""
        mag = torch.as_tensor(mag, dtype=D)
        return hr.half_ulp_bf16(mag) if self.bf16 else U * mag

    def store(self, t):
        """emulation: one store of a float32 value"""
        return t.to(torch.bfloat16).to(torch.float32) if self.bf16 else t


def acc(K):
    return (K + 2) * U


# ------------------------------------------------------------------------------------------------ cfg analysis
class Unit:
    def __init__(self, sec, kind, srcs, out, info):
        self.sec, self.kind, self.srcs, self.out, self.info = sec, kind, srcs, out, info

    def __repr__(self):
        return f"section {self.sec} {self.kind}"


class Graph:
    """Units of a Darknet cfg from oracle.yolo_oracle's layer table.  Nodes are named by the section whose output they are ("in": the image);
    a one-source route is the node of its source.  fused(i): conv i is read by the shortcut behind it alone, so a lowering may fold the add into
    the BatchNorm apply -- the unit then is conv + shortcut with node i + 1 as its output."""

    def __init__(self, layers, fuse=True):
        self.layers = layers
        n = len(layers)
        users = [[] for _ in range(n)]
        for i, L in enumerate(layers):
            t = L["type"]
            if t in ("convolutional", "upsample", "maxpool", "yolo") and i > 0:
                users[i - 1].append(i)
            elif t == "route":
                for v in L["layers"]:
                    users[i + v if v < 0 else v].append(i)
            elif t == "shortcut":
                users[i - 1].append(i)
                users[i + L["frm"] if L["frm"] < 0 else L["frm"]].append(i)
        self.canon = {}
        self.units = []
        skip = set()
        for i, L in enumerate(layers):
            t = L["type"]
            prev = self.canon[i - 1] if i else "in"
            if i in skip:
                continue
            if t == "convolutional":
                frm = None
                if fuse and L["bn"] and i + 1 < n and layers[i + 1]["type"] == "shortcut" and users[i] == [i + 1]:
                    f = layers[i + 1]["frm"]
                    f = i + 1 + f if f < 0 else f
                    if f != i:
                        frm = f
                if frm is not None:
                    self.units.append(Unit(i, "ConvBn", [prev, self.canon[frm]], i + 1, dict(L, resid=True)))
                    self.canon[i] = None
                    self.canon[i + 1] = i + 1
                    skip.add(i + 1)
                else:
                    self.units.append(Unit(i, "ConvBn" if L["bn"] else "ConvLinear", [prev], i, dict(L, resid=False)))
                    self.canon[i] = i
            elif t == "shortcut":
                f = i + L["frm"] if L["frm"] < 0 else L["frm"]
                self.units.append(Unit(i, "Shortcut", [prev, self.canon[f]], i, L))
                self.canon[i] = i
            elif t == "route":
                src = [self.canon[i + v if v < 0 else v] for v in L["layers"]]
                if len(src) == 1:
                    self.canon[i] = src[0]
                else:
                    self.units.append(Unit(i, "Concat", src, i, L))
                    self.canon[i] = i
            elif t in ("upsample", "maxpool"):
                self.units.append(Unit(i, "Upsample" if t == "upsample" else "MaxPool", [prev], i, L))
                self.canon[i] = i
            elif t == "yolo":
                self.units.append(Unit(i, "YoloHead", [prev], None, L))
                self.canon[i] = prev
        self.consumers = {}
        self.chan = {"in": layers[0]["cin"]}                 # true channels of every node
        for u in self.units:
            for k, s in enumerate(u.srcs):
                self.consumers.setdefault(s, []).append((u, k))
            if u.out is not None:
                self.chan[u.out] = (u.info["cout"] if u.kind in ("ConvBn", "ConvLinear") else
                                    sum(self.chan[s] for s in u.srcs) if u.kind == "Concat" else self.chan[u.srcs[0]])

    def fused_sections(self):
        return sorted(u.sec for u in self.units if u.kind == "ConvBn" and u.info["resid"])


def act_fn(t, act, slope):
    return F.leaky_relu(t, slope) if act == "leaky" else (F.relu(t) if act == "ReLU" else t)


# ------------------------------------------------------------------------------------------------ conv -> BatchNorm -> act (+ residual)
def _conv(x, w, L, b=None):
    return F.conv2d(x, w, b, stride=L["stride"], padding=L["pad"], dilation=L.get("dil", 1))


def _stat_bounds(y, e_y, eps):
    """bounds of mean / var / invstd of float64 y whose elements carry e_y -> mean, var, invstd, e_mean, e_invstd ([C] each)"""
    K = y.numel() // y.shape[1]
    dims = (0, 2, 3)
    mean, q = y.mean(dims), (y * y).mean(dims)
    var = y.var(dims, unbiased=False)
    e_mean = e_y.mean(dims) + acc(K) * y.abs().mean(dims)
    e_q = (2 * y.abs() * e_y + e_y * e_y).mean(dims) + acc(K) * q
    e_var = e_q + 2 * mean.abs() * e_mean + e_mean * e_mean
    inv = (var + eps).rsqrt()
    lo = (var + eps + e_var).rsqrt()
    hi = (var + eps - e_var).clamp_min(1e-300).rsqrt()
    e_inv = torch.maximum(hi - inv, inv - lo) + 4 * U * inv
    e_inv = torch.where(var + eps - e_var > 0, e_inv, torch.full_like(e_inv, float("inf")))
    return mean, var, inv, e_mean, e_inv


def _stat_gap(P, y_dev, mean, inv, stats, eps):
    """How far the statistics the device's backward uses may lie from those of its stored y in float64 (the reference's): with the device's own
    mean / invstd at hand -- inputs of the backward, audited against x by the forward -- the gap itself (+ 4 u); without, its bound from the one
    store of y between them."""
    if stats is not None:
        return (stats[0] - mean).abs() + 4 * U * mean.abs(), (stats[1] - inv).abs() + 4 * U * inv
    _, _, _, d_mean, d_inv = _stat_bounds(y_dev, P.rnd(y_dev.abs()), eps)
    return d_mean, d_inv


def convbn_forward(P, x, w, gamma, beta, resid, L, act, slope, eps=1e-5):
    """-> {name: (expected, bound)} for y, mean, invstd, z from the unit's inputs (float64 NCHW; w already as the plan holds it)"""
    c = lambda v: v.view(1, -1, 1, 1)       # noqa: E731
    y = _conv(x, w, L)
    K = w.shape[1] * w.shape[2] * w.shape[3]
    e_acc = acc(K) * _conv(x.abs(), w.abs(), L)
    e_y = e_acc + P.rnd(y.abs() + e_acc)
    mean, var, inv, e_mean, e_inv = _stat_bounds(y, e_acc, eps)
    t = c(gamma) * (y - c(mean)) * c(inv) + c(beta)
    e_t = c(gamma.abs()) * (c(inv) * (e_y + c(e_mean)) + (y - c(mean)).abs() * c(e_inv)) + 8 * U * (t.abs() + c(beta.abs()))
    z = act_fn(t, act, slope)
    if resid is not None:
        z = z + resid
        e_t = e_t + 2 * U * z.abs()
    e_z = e_t + P.rnd(z.abs() + e_t)
    return {"y": (y, e_y), "mean": (mean, e_mean), "invstd": (inv, e_inv), "z": (z, e_z)}


def convbn_backward(P, x, w, gamma, beta, y_dev, dz, L, act, slope, need_dx, eps=1e-5, stats=None):
    """-> {name: (expected, bound)} for dW, dgamma, dbeta, dx (and, for the emulation test, dy) from (x, the device's y, dz)"""
    c = lambda v: v.view(1, -1, 1, 1)       # noqa: E731
    K = y_dev.numel() // y_dev.shape[1]
    yl = y_dev.clone().requires_grad_(True)
    gl, bl = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    dims = (0, 2, 3)
    mean = yl.mean(dims)
    var = yl.var(dims, unbiased=False)
    inv = (var + eps).rsqrt()
    xhat = (yl - c(mean)) * c(inv)
    t = c(gl) * xhat + c(bl)
    z = act_fn(t, act, slope)
    dy, dgamma, dbeta = torch.autograd.grad(z, [yl, gl, bl], dz)
    # ---- magnitudes the bounds need
    with torch.no_grad():
        t, xhat, mean, inv = t.detach(), xhat.detach(), mean.detach(), inv.detach()
        d_mean, d_inv = _stat_gap(P, y_dev, mean, inv, stats, eps)
        e_xhat = c(inv) * c(d_mean) + (y_dev - c(mean)).abs() * c(d_inv) + 4 * U * xhat.abs()
        e_t = c(gamma.abs()) * e_xhat + 8 * U * (t.abs() + c(beta.abs()))
        sl = slope if act == "leaky" else 0.0
        kink = (t.abs() <= e_t) if act in ("leaky", "ReLU") else torch.zeros_like(t, dtype=torch.bool)
        g = dz * torch.where(t > 0, torch.ones_like(t), torch.full_like(t, sl)) if act in ("leaky", "ReLU") else dz
        e_g = torch.where(kink, (1 - sl) * dz.abs(), 4 * U * g.abs())
        e_dbeta = e_g.sum(dims) + acc(K) * g.abs().sum(dims)
        e_dgamma = ((e_g * xhat.abs() + g.abs() * e_xhat).sum(dims)
                    + acc(K) * inv * ((g * y_dev).abs().sum(dims) + mean.abs() * g.abs().sum(dims)))
        gi = c(gamma.abs() * inv)
        e_dy = (gi * (e_g + c(e_dbeta) / K + e_xhat * c(dgamma.abs()) / K + xhat.abs() * c(e_dgamma) / K)
                + dy.abs() * c(d_inv / inv)
                + 8 * U * gi * (g.abs() + c(dbeta.abs()) / K + c(dgamma.abs()) / K * c(inv) * (y_dev.abs() + c(mean.abs()))))
        e_dy = e_dy + P.rnd(dy.abs() + e_dy)
    out = {"dgamma": (dgamma, e_dgamma), "dbeta": (dbeta, e_dbeta), "dy": (dy, e_dy)}
    out.update(conv_backward(x, w, dy, e_dy, L, need_dx))
    return out


def conv_backward(x, w, dy, e_dy, L, need_dx):
    """dW and the contribution to dx of y = conv(x, w) for an output gradient dy known to e_dy"""
    def grads(xx, ww, gy):
        xx, ww = xx.clone().requires_grad_(True), ww.clone().requires_grad_(True)
        return torch.autograd.grad(_conv(xx, ww, L), [xx, ww], gy)
    dx, dw = grads(x, w, dy)
    ax, aw = grads(x.abs(), w.abs(), dy.abs())
    ex, ew = grads(x.abs(), w.abs(), e_dy) if e_dy is not None else (0.0, 0.0)
    Kw = dy.shape[0] * dy.shape[2] * dy.shape[3]
    Kx = w.shape[0] * w.shape[2] * w.shape[3]
    out = {"dW": (dw, ew + acc(Kw) * aw)}
    if need_dx:
        out["dx"] = (dx, ex + acc(Kx) * ax)
    return out


def convlinear(P, x, w, b, dy, L, need_dx=True):
    """head conv with bias: y, and from the device's dy: dW, dbias, dx"""
    y = _conv(x, w, L, b)
    K = w.shape[1] * w.shape[2] * w.shape[3]
    e_acc = acc(K) * (_conv(x.abs(), w.abs(), L) + b.abs().view(1, -1, 1, 1))
    out = {"y": (y, e_acc + P.rnd(y.abs() + e_acc))}
    if dy is not None:
        out.update(conv_backward(x, w, dy, None, L, need_dx))
        Kb = dy.shape[0] * dy.shape[2] * dy.shape[3]
        out["dbias"] = (dy.sum((0, 2, 3)), acc(Kb) * dy.abs().sum((0, 2, 3)))
    return out


# ------------------------------------------------------------------------------------------------ data movement units
def maxpool(x, dz, L):
    k, st = L["k"], L["stride"]
    zero_pad = k == 2 and st == 1
    xl = x.clone().requires_grad_(True)
    xp = F.pad(xl, (0, 1, 0, 1)) if zero_pad else xl
    pad = (k - 1) // 2
    z = F.max_pool2d(xp, k, st, pad)
    out = {"z": (z.detach(), torch.zeros_like(z))}
    if dz is not None:
        dx, = torch.autograd.grad(z, xl, dz, retain_graph=True)
        with torch.no_grad():                                   # ties: either position of a window whose maximum is attained twice
            xq = F.pad(x, (0, 1, 0, 1)) if zero_pad else F.pad(x, (pad,) * 4, value=-float("inf"))
            B, C, Hq, Wq = xq.shape
            cols = F.unfold(xq, k, stride=st).view(B, C, k * k, -1)
            eq = cols == cols.max(2, keepdim=True).values
            tied = eq & (eq.sum(2, keepdim=True) > 1)
            wgt = tied.to(D) * dz.abs().reshape(B, C, 1, -1)
            e = F.fold(wgt.view(B, C * k * k, -1), (Hq, Wq), k, stride=st)
            e = e[:, :, :x.shape[2], :x.shape[3]] if zero_pad else e[:, :, pad:pad + x.shape[2], pad:pad + x.shape[3]]
        k2 = k * k if st < k else 1                            # overlapping windows: up to k^2 gradients meet in one input element
        mag, = torch.autograd.grad(z, xl, dz.abs())
        out["dx"] = (dx, e + (acc(k2) * mag if k2 > 1 else 0.0))
    return out


def upsample(x, dz, L):
    sc = L["scale"]
    xl = x.clone().requires_grad_(True)
    z = F.interpolate(xl, scale_factor=sc, mode="nearest")
    out = {"z": (z.detach(), torch.zeros_like(z))}
    if dz is not None:
        dx, = torch.autograd.grad(z, xl, dz)
        out["dx"] = (dx, acc(sc * sc) * F.avg_pool2d(dz.abs(), sc) * sc * sc)
    return out


def yolo_head(P, lg, L, classes, cfg_h, targets, consts, gscale=1.0):
    """-> loss (value, bound), parts, dlogits from the device's logits; float32 evaluation of the same expression gives the error scale"""
    def run(dt):
        s = lg.to(dt).clone().requires_grad_(True)
        loss, parts = yo.yolo_layer(s, L["anchors"], classes, cfg_h, targets, **consts)
        loss.backward()
        return loss.detach().to(D), parts.to(D), s.grad.to(D)
    l64, p64, g64 = run(D)
    l32, p32, g32 = run(torch.float32)
    g64 = g64 * gscale
    b_g = hr.bound(hr.maxabs(g32 * gscale - g64), hr.maxabs(g64))
    e_g = torch.full_like(g64, b_g)
    e_g = e_g + P.rnd(g64.abs() + e_g)
    return {"loss": (l64, torch.tensor(hr.bound(abs(float(l32 - l64)), abs(float(l64))), dtype=D)),
            "parts": (p64, torch.stack([torch.tensor(hr.bound(abs(float(a - b)), abs(float(b))), dtype=D) for a, b in zip(p32, p64)])),
            "dx": (g64, e_g)}


def yolo_decode(P, lg, L, classes, cfg_h):
    o64 = yo.yolo_layer(lg.to(D), L["anchors"], classes, cfg_h)
    o32 = yo.yolo_layer(lg.to(torch.float32), L["anchors"], classes, cfg_h).to(D)
    return {"rows": (o64, torch.full_like(o64, hr.bound(hr.maxabs(o32 - o64), 0.0)) + 8 * 4 * U * o64.abs())}


# ------------------------------------------------------------------------------------------------ node gradients
def node_grad(P, contribs):
    """contribs: [(expected, bound, computed)] of every consumer -> (expected total, bound) of the node's gradient buffer"""
    n = len(contribs)
    c = sum(1 for _, _, comp in contribs if comp)
    tot = sum(v for v, _, _ in contribs)
    e = sum(b for _, b, _ in contribs)
    if n == 1 and c == 0:
        return tot, torch.zeros_like(tot)
    mag = sum(v.abs() + b for v, b, _ in contribs)
    return tot, e + (c + n - 1) * P.rnd(mag)


# ------------------------------------------------------------------------------------------------ comparison
class Miss(AssertionError):
    pass


def ratio(got, want, bound):
    """largest |got - want| / bound (0/0 = 0, x/0 = inf) and where -> (ratio, index tuple, got, want, bound at that element)"""
    got, want = got.to(D), want.to(D)
    bound = torch.as_tensor(bound, dtype=D).expand_as(want)
    err = (got - want).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    if r.numel() == 0:
        return 0.0, (), 0.0, 0.0, 0.0
    k = int(r.reshape(-1).argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(k), r.shape)) if r.dim() else ()
    return float(r.reshape(-1)[k]), idx, float(got.reshape(-1)[k]), float(want.reshape(-1)[k]), float(bound.reshape(-1)[k])


class Report:
    """collects error / bound per (unit, tensor); `misses` are the comparisons above 1"""

    def __init__(self):
        self.rows = []

    def check(self, units, name, got, want, bound):
        """units: the unit the comparison belongs to, or -- for a node's gradient -- every consumer that contributes to it"""
        units = tuple(units) if isinstance(units, (list, tuple)) else (units,)
        r = ratio(got, want, bound)
        self.rows.append((units, name) + r)
        return r[0]

    @property
    def misses(self):
        return [r for r in self.rows if not r[2] <= 1.0]

    def missed_sections(self):
        """per miss, the set of sections it may be charged to"""
        return [frozenset(u.sec for u in r[0]) for r in self.misses]

    def worst_by_kind(self):
        w = {}
        for r in self.rows:
            k = ("node", "grad") if r[1].startswith("grad of") else (r[0][0].kind, r[1].split("(")[0])
            if math.isfinite(r[2]) and r[2] > w.get(k, -1.0):
                w[k] = r[2]
        return w

    def format_misses(self, limit=12):
        lines = []
        for unit, name, r, idx, got, want, bound in sorted(self.misses, key=lambda v: -v[2] if math.isfinite(v[2]) else -1e300)[:limit]:
            lines.append(f"{' / '.join(map(repr, unit))} {name} at {idx}: got {got!r} want {want!r} |err| {abs(got - want):.3e} bound {bound:.3e} "
                         f"error/bound {r:.3g}")
        return "\n".join(lines)

    def assert_clean(self, what=""):
        if self.misses:
            raise Miss(f"{what}: {len(self.misses)} comparison(s) above their bound\n" + self.format_misses())


# ------------------------------------------------------------------------------------------------ the audit of one Darknet step
class Tensors:
    """What an audit reads, as float64 NCHW CPU tensors (true channels only).  The GPU test fills it from the plan; the host tests from an
    emulation or from the reference itself."""

    def __init__(self):
        self.act = {}        # node -> activation
        self.grad = {}       # node -> gradient buffer (absent: the node has none)
        self.y = {}          # conv section -> raw conv output
        self.mean, self.invstd = {}, {}
        self.pgrad = {}      # oracle parameter name -> gradient
        self.out7 = None
        self.rows = None     # eval plans: decoded rows


def audit_darknet(P, graph, params, tens, targets, hyper, report, train=True, gscale=1.0, bn_eval=False):
    """Audits every unit of `graph` against `tens`.  params: oracle-style names -> float64 master tensors.  hyper: dict(classes, cfg_h, slope,
    act, consts).  train=False: forward only (eval plans: running statistics, decoded rows)."""
    act, slope = hyper["act"], hyper["slope"]
    contribs = {}
    loss_w, loss_b, parts_w, parts_b = 0.0, 0.0, 0.0, 0.0
    rows = []
    for u in graph.units:
        L, i = u.info, u.sec
        ins = [tens.act[s] for s in u.srcs]
        if train and u.out is not None and u.out not in tens.grad:
            raise Miss(f"{u!r}: its output node {u.out} has no gradient buffer after a training step (consumers: {graph.consumers.get(u.out)})")
        dz = tens.grad[u.out] if (train and u.out is not None) else None
        if u.kind == "ConvBn":
            w = P.weights(params[f"conv{i}.weight"])
            gamma, beta = params[f"bn{i}.weight"], params[f"bn{i}.bias"]
            resid = ins[1] if L["resid"] else None
            if bn_eval:
                y = _conv(ins[0], w, L)
                K = w.shape[1] * w.shape[2] * w.shape[3]
                c = lambda v: v.view(1, -1, 1, 1)       # noqa: E731
                rm, rv = params[f"bn{i}.running_mean"], params[f"bn{i}.running_var"]
                sc = gamma * (rv + 1e-5).rsqrt()
                sh = beta - rm * sc
                t = y * c(sc) + c(sh)
                e_acc = acc(K) * _conv(ins[0].abs(), w.abs(), L)
                # one launch: no store of y; two passes: one.  Both admitted: e_y as in training
                e_y = e_acc + P.rnd(y.abs() + e_acc)
                e_t = c(sc.abs()) * e_y + 8 * U * (t.abs() + y.abs() * c(sc.abs()) + c(sh.abs()) + c((rm * sc).abs()))
                z = act_fn(t, act, slope)
                if resid is not None:
                    # the conv's store path stages its tile in the plan's type BEFORE the residual is added (csrc/conv_gemm.h epilogue): the folded
                    # add rounds act(t) and then the sum, like the conv + shortcut pair it replaces (found by this audit: 2.3 x the one-store bound)
                    e_t = e_t + P.rnd(z.abs() + e_t)
                    z = z + resid
                    e_t = e_t + 2 * U * z.abs()
                report.check(u, "z", tens.act[u.out], z, e_t + P.rnd(z.abs() + e_t))
                continue
            f = convbn_forward(P, ins[0], w, gamma, beta, resid, L, act, slope)
            report.check(u, "y", tens.y[i], *f["y"])
            report.check(u, "mean", tens.mean[i], *f["mean"])
            report.check(u, "invstd", tens.invstd[i], *f["invstd"])
            report.check(u, "z", tens.act[u.out], *f["z"])
            if dz is None:
                continue
            need_dx = u.srcs[0] != "in"
            b = convbn_backward(P, ins[0], w, gamma, beta, tens.y[i], dz, L, act, slope, need_dx, stats=(tens.mean[i], tens.invstd[i]))
            report.check(u, "dW", tens.pgrad[f"conv{i}.weight"], *b["dW"])
            report.check(u, "dgamma", tens.pgrad[f"bn{i}.weight"], *b["dgamma"])
            report.check(u, "dbeta", tens.pgrad[f"bn{i}.bias"], *b["dbeta"])
            if need_dx:
                contribs.setdefault(u.srcs[0], []).append((u, b["dx"][0], b["dx"][1], True))
            if resid is not None:
                contribs.setdefault(u.srcs[1], []).append((u, dz, torch.zeros_like(dz), False))
        elif u.kind == "ConvLinear":
            w, bias = P.weights(params[f"conv{i}.weight"]), params[f"conv{i}.bias"]
            r = convlinear(P, ins[0], w, bias, dz, L)
            report.check(u, "y", tens.act[u.out], *r["y"])
            if dz is not None:
                report.check(u, "dW", tens.pgrad[f"conv{i}.weight"], *r["dW"])
                report.check(u, "dbias", tens.pgrad[f"conv{i}.bias"], *r["dbias"])
                contribs.setdefault(u.srcs[0], []).append((u, r["dx"][0], r["dx"][1], True))
        elif u.kind == "Shortcut":
            z = ins[0] + ins[1]
            report.check(u, "z", tens.act[u.out], z, P.rnd(z.abs()))
            if dz is not None:
                for s in u.srcs:
                    contribs.setdefault(s, []).append((u, dz, torch.zeros_like(dz), False))
        elif u.kind == "Concat":
            z = torch.cat(ins, 1)
            report.check(u, "z", tens.act[u.out], z, torch.zeros_like(z))
            if dz is not None:
                off = 0
                for s, t in zip(u.srcs, ins):
                    part = dz[:, off:off + t.shape[1]]
                    contribs.setdefault(s, []).append((u, part, torch.zeros_like(part), False))
                    off += t.shape[1]
        elif u.kind in ("MaxPool", "Upsample"):
            r = (maxpool if u.kind == "MaxPool" else upsample)(ins[0], dz, L)
            report.check(u, "z", tens.act[u.out], *r["z"])
            if dz is not None:
                contribs.setdefault(u.srcs[0], []).append((u, r["dx"][0], r["dx"][1], True))
        elif u.kind == "YoloHead":
            if not train:
                rows.append(yolo_decode(P, ins[0], L, hyper["classes"], hyper["cfg_h"])["rows"])
                continue
            r = yolo_head(P, ins[0], L, hyper["classes"], hyper["cfg_h"], targets, hyper["consts"], gscale)
            loss_w, loss_b = loss_w + r["loss"][0], loss_b + r["loss"][1]
            parts_w, parts_b = parts_w + r["parts"][0], parts_b + r["parts"][1]
            contribs.setdefault(u.srcs[0], []).append((u, r["dx"][0], r["dx"][1], True))
            u_head = u
    if not train:
        if rows and tens.rows is not None:
            want, bnd = torch.cat([r[0] for r in rows], 1), torch.cat([r[1] for r in rows], 1)
            report.check(graph.units[-1], "rows", tens.rows, want, bnd)
        return
    report.check(u_head, "loss", tens.out7[0], loss_w, loss_b + 4 * U * abs(loss_w))
    report.check(u_head, "parts", tens.out7[1:], parts_w, parts_b + 4 * U * parts_w.abs())
    # node gradients: a miss is charged to every consumer of the node (any of their contributions, or their accumulation, may be the wrong one)
    for node, cl in contribs.items():
        if node == "in":
            continue
        want, bnd = node_grad(P, [(v, b, comp) for _, v, b, comp in cl])
        report.check([c[0] for c in cl], f"grad of node {node}", tens.grad[node], want, bnd)


# ------------------------------------------------------------------------------------------------ exact decomposition (host test)
def decompose_darknet(graph, params, x, targets, hyper):
    """Runs the units on their OWN float64 outputs and sums the contributions -> Tensors (activations, gradients of every node, parameter
    gradients, out7).  Compared with DarknetOracle's autograd by tests/test_plan_audit_host.py."""
    P = Prec(False)
    P.weights = lambda w: w.to(D)
    tens = Tensors()
    tens.act["in"] = x
    act, slope = hyper["act"], hyper["slope"]
    loss, parts = 0.0, 0.0
    for u in graph.units:
        L, i = u.info, u.sec
        ins = [tens.act[s] for s in u.srcs]
        if u.kind == "ConvBn":
            f = convbn_forward(P, ins[0], params[f"conv{i}.weight"], params[f"bn{i}.weight"], params[f"bn{i}.bias"],
                               ins[1] if L["resid"] else None, L, act, slope)
            tens.y[i], tens.mean[i], tens.invstd[i], tens.act[u.out] = f["y"][0], f["mean"][0], f["invstd"][0], f["z"][0]
        elif u.kind == "ConvLinear":
            tens.act[u.out] = convlinear(P, ins[0], params[f"conv{i}.weight"], params[f"conv{i}.bias"], None, L)["y"][0]
        elif u.kind == "Shortcut":
            tens.act[u.out] = ins[0] + ins[1]
        elif u.kind == "Concat":
            tens.act[u.out] = torch.cat(ins, 1)
        elif u.kind == "MaxPool":
            tens.act[u.out] = maxpool(ins[0], None, L)["z"][0]
        elif u.kind == "Upsample":
            tens.act[u.out] = upsample(ins[0], None, L)["z"][0]
    pend = {}
    for u in reversed(graph.units):
        L, i = u.info, u.sec
        ins = [tens.act[s] for s in u.srcs]
        if u.kind == "YoloHead":
            r = yolo_head(P, ins[0], L, hyper["classes"], hyper["cfg_h"], targets, hyper["consts"])
            loss, parts = loss + r["loss"][0], parts + r["parts"][0]
            pend.setdefault(u.srcs[0], []).append(r["dx"][0])
            continue
        dz = sum(pend[u.out])
        tens.grad[u.out] = dz
        if u.kind == "ConvBn":
            need_dx = u.srcs[0] != "in"
            b = convbn_backward(P, ins[0], params[f"conv{i}.weight"], params[f"bn{i}.weight"], params[f"bn{i}.bias"], tens.y[i], dz, L, act,
                                slope, need_dx)
            tens.pgrad[f"conv{i}.weight"], tens.pgrad[f"bn{i}.weight"], tens.pgrad[f"bn{i}.bias"] = b["dW"][0], b["dgamma"][0], b["dbeta"][0]
            if need_dx:
                pend.setdefault(u.srcs[0], []).append(b["dx"][0])
            if L["resid"]:
                pend.setdefault(u.srcs[1], []).append(dz)
        elif u.kind == "ConvLinear":
            r = convlinear(P, ins[0], params[f"conv{i}.weight"], params[f"conv{i}.bias"], dz, L)
            tens.pgrad[f"conv{i}.weight"], tens.pgrad[f"conv{i}.bias"] = r["dW"][0], r["dbias"][0]
            pend.setdefault(u.srcs[0], []).append(r["dx"][0])
        elif u.kind == "Shortcut":
            for s in u.srcs:
                pend.setdefault(s, []).append(dz)
        elif u.kind == "Concat":
            off = 0
            for s, t in zip(u.srcs, ins):
                pend.setdefault(s, []).append(dz[:, off:off + t.shape[1]])
                off += t.shape[1]
        else:
            r = (maxpool if u.kind == "MaxPool" else upsample)(ins[0], dz, L)
            pend.setdefault(u.srcs[0], []).append(r["dx"][0])
    tens.out7 = torch.cat([torch.as_tensor(loss, dtype=D).view(1), parts])
    return tens


# ------------------------------------------------------------------------------------------------ float32 / bf16-store emulation (host test)
def _pool_f32(x, L):
    k, st = L["k"], L["stride"]
    if k == 2 and st == 1:
        x = F.pad(x, (0, 1, 0, 1))
    return F.max_pool2d(x, k, st, (k - 1) // 2)


def emulate_darknet(P, graph, params, x, targets, hyper):
    """A plan as the kernels are specified, in torch on the CPU: float32 arithmetic, stores (bf16 for bf16 plans) at the named points -- y, z, dy,
    every gradient contribution and every accumulation into a gradient buffer.  -> Tensors, audited by audit_darknet like a device's."""
    f32 = torch.float32
    st = P.store
    act, slope = hyper["act"], hyper["slope"]
    c = lambda v: v.view(1, -1, 1, 1)       # noqa: E731
    A, Y, MEAN, INV, G, PG = {}, {}, {}, {}, {}, {}
    A["in"] = st(x.to(f32))
    W = {k: st(v.to(f32)) if k.endswith("weight") and k.startswith("conv") else v.to(f32) for k, v in params.items()}
    for u in graph.units:
        L, i = u.info, u.sec
        ins = [A[s] for s in u.srcs]
        if u.kind == "ConvBn":
            y32 = _conv(ins[0], W[f"conv{i}.weight"], L)
            mean = y32.mean((0, 2, 3))
            var = ((y32 * y32).mean((0, 2, 3)).double() - mean.double() ** 2)
            inv = (var + 1e-5).rsqrt().to(f32)
            Y[i], MEAN[i], INV[i] = st(y32), mean, inv
            scale = W[f"bn{i}.weight"] * inv
            shift = W[f"bn{i}.bias"] - mean * scale
            z = act_fn(Y[i] * c(scale) + c(shift), act, slope)
            A[u.out] = st(z + ins[1] if L["resid"] else z)
        elif u.kind == "ConvLinear":
            A[u.out] = st(_conv(ins[0], W[f"conv{i}.weight"], L, W[f"conv{i}.bias"]))
        elif u.kind == "Shortcut":
            A[u.out] = st(ins[0] + ins[1])
        elif u.kind == "Concat":
            A[u.out] = torch.cat(ins, 1)
        elif u.kind == "MaxPool":
            A[u.out] = _pool_f32(ins[0], L)
        elif u.kind == "Upsample":
            A[u.out] = F.interpolate(ins[0], scale_factor=L["scale"], mode="nearest")
    loss, parts = 0.0, 0.0

    def add(node, v, computed):
        if node == "in":
            return
        v = st(v) if computed else v
        G[node] = v if node not in G else st(G[node] + v)
    for u in reversed(graph.units):
        L, i = u.info, u.sec
        ins = [A[s] for s in u.srcs]
        if u.kind == "YoloHead":
            s = ins[0].clone().requires_grad_(True)
            l, p = yo.yolo_layer(s, L["anchors"], hyper["classes"], hyper["cfg_h"], targets, **hyper["consts"])
            l.backward()
            loss, parts = loss + l.detach(), parts + p
            add(u.srcs[0], s.grad, True)
            continue
        dz = G[u.out]
        if u.kind == "ConvBn":
            K = Y[i].numel() // Y[i].shape[1]
            scale = W[f"bn{i}.weight"] * INV[i]
            shift = W[f"bn{i}.bias"] - MEAN[i] * scale
            t = Y[i] * c(scale) + c(shift)
            sl = slope if act == "leaky" else 0.0
            g = dz * torch.where(t > 0, torch.ones_like(t), torch.full_like(t, sl)) if act in ("leaky", "ReLU") else dz
            xhat = (Y[i] - c(MEAN[i])) * c(INV[i])
            dbeta, dgamma = g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))
            dy = st(c(scale) * (g - c(dbeta) / K - xhat * c(dgamma) / K))
            PG[f"bn{i}.weight"], PG[f"bn{i}.bias"] = dgamma, dbeta
            xx, ww = ins[0].clone().requires_grad_(True), W[f"conv{i}.weight"].clone().requires_grad_(True)
            dx, dw = torch.autograd.grad(_conv(xx, ww, L), [xx, ww], dy)
            PG[f"conv{i}.weight"] = dw
            add(u.srcs[0], dx, True)
            if L["resid"]:
                add(u.srcs[1], dz, False)
        elif u.kind == "ConvLinear":
            xx, ww = ins[0].clone().requires_grad_(True), W[f"conv{i}.weight"].clone().requires_grad_(True)
            dx, dw = torch.autograd.grad(_conv(xx, ww, L), [xx, ww], dz)
            PG[f"conv{i}.weight"], PG[f"conv{i}.bias"] = dw, dz.sum((0, 2, 3))
            add(u.srcs[0], dx, True)
        elif u.kind == "Shortcut":
            for s in u.srcs:
                add(s, dz, False)
        elif u.kind == "Concat":
            off = 0
            for s, t in zip(u.srcs, ins):
                add(s, dz[:, off:off + t.shape[1]], False)
                off += t.shape[1]
        elif u.kind == "MaxPool":                                 # float32 scatter-add of the window gradients (overlapping windows meet in fp32)
            xx = ins[0].clone().requires_grad_(True)
            add(u.srcs[0], torch.autograd.grad(_pool_f32(xx, L), xx, dz)[0], True)
        else:                                                     # float32 sum of the scale^2 gradients
            sc = L["scale"]
            add(u.srcs[0], F.avg_pool2d(dz, sc, divisor_override=1), True)
    tens = Tensors()
    d = lambda m: {k: v.to(D) for k, v in m.items()}       # noqa: E731
    tens.act, tens.grad, tens.y, tens.mean, tens.invstd, tens.pgrad = d(A), d(G), d(Y), d(MEAN), d(INV), d(PG)
    tens.out7 = torch.cat([torch.as_tensor(loss).view(1), parts]).to(D)
    return tens


# ------------------------------------------------------------------------------------------------ the audit nets
_HEAD = ("[net]\nwidth={w}\nheight={h}\nonnx_height={h}\nclasses={classes}\nchannels=3\n"
         "yolo_masks={masks}\nyolo_scales={scales}\nvalidate_uri=dataset/validate.csv\ntrain_uri=dataset/train.csv\n"
         "weights_uri=none\nstart_weights_dim={swd}\nnum_train_images=-1\nnum_validate_images=-1\nleaky_slope=0.1\n"
         "conv_activation=leaky\nbuild_targets_ignore_thresh=0.5\nconf_thresh=0.8\nnms_thresh=0.25\niou_thresh=0.5\n\n")
ANCHOR_ROW = '"10,13|16,30|33,23|30,61|62,45|59,119|116,90|156,198|373,326"\n'


def write_compact_cfg(tmp, classes=2, h=128, w=160):
    """The wiring pattern of yolo_baseline at widths 64..512 (the first conv keeps yolo_baseline's 32 filters: the two-pass first-conv kernel is
    compiled for that width): first 3x3 conv, stride-2 3x3 convs, 1x1/3x3 residual pairs -- the last 3x3 conv of
    the pair at sections 17-19 is read by the route at section 31 as well, so its shortcut is an explicit add; every other pair folds the add into
    the BatchNorm apply --, three heads with route -4, 1x1, upsample and a two-source route."""
    import os

    def conv(f, k, s=1):
        return f"[convolutional]\nfilters={f}\nsize={k}\nstride={s}\n\n"

    def res(c):
        return conv(c // 2, 1) + conv(c, 3) + "[shortcut]\nfrom=-3\n\n"
    body = conv(32, 3) + conv(128, 3, 2) + res(128)                     # 0, 1, 2-4      (H/2)
    body += conv(128, 3, 2) + res(128) + res(128)                       # 5, 6-8, 9-11   (H/4)
    body += conv(256, 3, 2) + res(256)                                  # 12, 13-15      (H/8)
    body += conv(512, 3, 2) + res(512)                                  # 16, 17-19      (H/16)
    body += conv(512, 3, 2) + res(512)                                  # 20, 21-23      (H/32)
    body += conv(256, 1) + conv(512, 3) + conv("preyolo", 1) + "[yolo]\n\n"                    # 24 25 26 27
    body += "[route]\nlayers=-4\n\n" + conv(128, 1) + "[upsample]\nstride=2\n\n[route]\nlayers=-1, 18\n\n"    # 28 29 30 31
    body += conv(128, 1) + conv(256, 3) + conv("preyolo", 1) + "[yolo]\n\n"                    # 32 33 34 35
    body += "[route]\nlayers=-4\n\n" + conv(64, 1) + "[upsample]\nstride=2\n\n[route]\nlayers=-1, 15\n\n"     # 36 37 38 39
    body += conv(128, 1) + conv(256, 3) + conv("preyolo", 1) + "[yolo]\n"                      # 40 41 42 43
    os.makedirs(os.path.join(tmp, "dataset"), exist_ok=True)
    with open(os.path.join(tmp, "dataset", "train.csv"), "w") as f:
        f.write(ANCHOR_ROW)
    path = os.path.join(tmp, "compact.cfg")
    n = 3 * (5 + classes)
    with open(path, "w") as f:
        f.write(_HEAD.format(w=w, h=h, classes=classes, masks="6,7,8|3,4,5|0,1,2", scales="32,16,8", swd=f"{n},{n},{n}") + body)
    return path


def compact_targets():
    """[3, 4, 5]: image 0 three boxes, image 1 none, image 2 one box"""
    g = torch.Generator().manual_seed(7)
    t = torch.zeros(3, 4, 5)
    for b, n in ((0, 3), (2, 1)):
        t[b, :n, 0] = torch.randint(0, 2, (n,), generator=g).float()
        t[b, :n, 1:3] = torch.rand(n, 2, generator=g) * 0.9 + 0.05
        t[b, :n, 3:5] = torch.rand(n, 2, generator=g) * 0.28 + 0.05
    return t


def oracle_params(orc, seed):
    """float64 copies of DarknetOracle.init_params(seed) with non-trivial running statistics"""
    orc.init_params(seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in list(orc.params):
        if k.endswith("running_mean"):
            orc.params[k] = (torch.rand(orc.params[k].shape, generator=g) - 0.5) * 0.4
        if k.endswith("running_var"):
            orc.params[k] = torch.rand(orc.params[k].shape, generator=g) * 1.5 + 0.5
    return {k: v.to(D) for k, v in orc.params.items()}


def hyper_of(orc):
    return dict(classes=orc.classes, cfg_h=orc.cfg_h, slope=orc.slope, act=orc.act, consts=orc.consts)
