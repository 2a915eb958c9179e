"""float64 references of the two loss heads (csrc/yolo_head.hip, csrc/rektnet_head.hip) for tests/test_gpu_heads.py.

Every function takes a torch dtype and evaluates ONE torch-CPU expression in it: float64 is the reference, the same call in float32 gives
``e32``, the error a correct fp32 evaluation of the expression makes on the very inputs of the case.  The bound of every comparison is
``bound(e32, scale)`` below, so no tolerance depends on what the kernels return.

  yolo_train / yolo_eval      oracle.yolo_oracle.yolo_layer (pinned to the reference project by tests/test_oracle_golden.py) + autograd
  yolo_layer_bce              the same layer with nn.BCELoss / nn.MSELoss as the reference project writes it: its backward is finite
                              when sigmoid() rounds to 0 or 1, the oracle's hand-written clamp(log()) is not
  softargmax / softargmax_bwd torch.softmax + linspace (oracle.rektnet_oracle.keypoint_forward's tail) + autograd
  cross_ratio                 oracle.rektnet_oracle.cross_ratio_loss + autograd, upstream gradients of the two parts as weights

tests/test_head_refs.py pins this module to the reference project's recorded outputs.
"""
import torch
import torch.nn.functional as F

from oracle import rektnet_oracle as ro
from oracle import yolo_oracle as yo

U = 2.0 ** -24                      # unit roundoff of fp32
WEIGHTS = dict(ignore_thres=0.5, xy_loss=2.0, wh_loss=1.6, object_loss=0.1, no_object_loss=25.0)
LOSS_TYPES = ("l2_softargmax", "l2_heatmap", "l1_softargmax")      # mdcv_cross_ratio_loss loss_type 0, 1, 2


def bound(e32, scale):
    """8 max(e32, 4 u scale): 8 = device expf / logf at a few ulp where libm is at 1/2 ulp, and another summation order; the floor of
    4 ulp of the largest reference magnitude keeps the bound alive where the fp32 evaluation happens to be exact"""
    return 8.0 * max(float(e32), 4.0 * U * float(scale))


def maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0


def half_ulp_bf16(x):
    """half a unit in the last place of bf16 (8 significand bits) at magnitude x >= 0: 2^(floor(log2 x) - 8), between 2^-9 x and 2^-8 x"""
    _, e = torch.frexp(x)
    return torch.where(x > 0, torch.ldexp(torch.ones_like(x), e - 9), torch.zeros_like(x))


# ------------------------------------------------------------------------------------------------ YOLO head
def yolo_anchors(stride):
    """anchor triple of the head with this stride, in pixels (models.py:13 vanilla_anchor_list, as tests/golden/make_golden.py slices it)"""
    return yo.VANILLA_ANCHORS[{32: slice(6, 9), 16: slice(3, 6), 8: slice(0, 3)}[stride]]


def scaled_anchors(anchors_px, stride):
    return torch.tensor([(aw / stride, ah / stride) for aw, ah in anchors_px], dtype=torch.float32)       # as yolo_layer builds them


def yolo_targets(B, T, gen, cls_hi=1, min_real=1):
    """[B,T,5] like make_golden.synth_targets: n in [min_real, T] real rows then zero padding rows; centres in (0.01, 0.99)"""
    t = torch.zeros(B, T, 5)
    for b in range(B):
        n = int(torch.randint(min_real, T + 1, (1,), generator=gen))
        t[b, :n, 0] = torch.randint(0, cls_hi, (n,), generator=gen).float()
        t[b, :n, 1:3] = torch.rand(n, 2, generator=gen) * 0.98 + 0.01
        t[b, :n, 3:5] = torch.rand(n, 2, generator=gen) * 0.28 + 0.02
    return t


class _Sigmoid(torch.autograd.Function):
    """torch.sigmoid with a value that does not depend on the host: forward 1/(1+exp(-x)) for x >= 0 and exp(x)/(1+exp(x)) for x < 0,
    backward grad p (1 - p) as torch.sigmoid's.  torch.sigmoid(-95.) in fp32 is 0 where the CPU kernel evaluates 1/(1+exp(95)) = 1/inf
    (seen on an AVX-512 build) and the denormal 5.5e-42 elsewhere; exp(-95.) is that denormal everywhere, and it is the rounded true value."""

    @staticmethod
    def forward(ctx, x):
        e = torch.exp(-x.abs())
        p = torch.where(x >= 0, 1 / (1 + e), e / (1 + e))
        ctx.save_for_backward(p)
        return p

    @staticmethod
    def backward(ctx, g):
        p, = ctx.saved_tensors
        return g * (1 - p) * p


def stable_sigmoid(x):
    return _Sigmoid.apply(x)


def yolo_layer_bce(sample, anchors_px, num_classes, cfg_height, targets, ignore_thres=0.5, xy_loss=2.0, wh_loss=1.6, object_loss=0.1,
                   no_object_loss=25.0):
    """training branch of yolo_oracle.yolo_layer with F.mse_loss / F.binary_cross_entropy on the masked cells (models.py:186-205)"""
    A = len(anchors_px)
    B, _, Gh, Gw = sample.shape
    stride = cfg_height / Gh
    p = sample.view(B, A, 5 + num_classes, Gh, Gw).permute(0, 1, 3, 4, 2)
    sx, sy, rw, rh, conf = stable_sigmoid(p[..., 0]), stable_sigmoid(p[..., 1]), p[..., 2], p[..., 3], stable_sigmoid(p[..., 4])
    m, cm, tx, ty, tw, th, tconf, _ = yo.build_targets(targets, scaled_anchors(anchors_px, stride), A, num_classes, Gh, Gw, ignore_thres)
    pos, neg = m.bool(), (cm - m).bool()
    d = sample.dtype
    lx = xy_loss * F.mse_loss(sx[pos], tx[pos].to(d))
    ly = xy_loss * F.mse_loss(sy[pos], ty[pos].to(d))
    lw = wh_loss * F.mse_loss(rw[pos], tw[pos].to(d))
    lh = wh_loss * F.mse_loss(rh[pos], th[pos].to(d))
    lno = no_object_loss * F.binary_cross_entropy(conf[neg], tconf[neg].to(d))
    lob = object_loss * F.binary_cross_entropy(conf[pos], tconf[pos].to(d))
    loss = lx + ly + lw + lh + lno + lob
    return loss, torch.stack([v.detach() for v in (lx, ly, lw, lh, lob, lno)])


def yolo_train(sample, anchors_px, C, cfg_h, targets, dtype, layer=yo.yolo_layer):
    """-> loss (0-d), parts [6], dsample [B, A(5+C), Gh, Gw], all float64 tensors holding the values computed in `dtype`"""
    s = sample.detach().to(dtype).clone().requires_grad_(True)
    loss, parts = layer(s, anchors_px, C, cfg_h, targets, **WEIGHTS)
    loss.backward()
    return loss.detach().double(), parts.double(), s.grad.double()


def yolo_eval(sample, anchors_px, C, cfg_h, dtype):
    """-> [B, A Gh Gw, 5+C] float64 (values computed in `dtype`)"""
    return yo.yolo_layer(sample.detach().to(dtype), anchors_px, C, cfg_h).double()


def yolo_masks(targets, anchors_px, C, Gh, Gw, stride):
    """-> mask, conf_mask - mask as bool [B,A,Gh,Gw] (positive cells, no-object cells)"""
    m, cm = yo.build_targets(targets, scaled_anchors(anchors_px, stride), len(anchors_px), C, Gh, Gw, WEIGHTS["ignore_thres"])[:2]
    return m.bool(), (cm - m).bool()


# ------------------------------------------------------------------------------------------------ key-point head
def softargmax(z, dtype):
    """z [B,K,H,W] -> heat-map [B,K,H,W], points [B,K,2] in (x, y) order (keypoint_net.py:46-56,68-70), in `dtype`"""
    B, K, H, W = z.shape
    z = z.to(dtype)
    hm = torch.softmax(z.reshape(-1, H * W), 1).view(B, K, H, W)
    vy = torch.linspace(0, (H - 1.0) / H, H, dtype=dtype)
    vx = torch.linspace(0, (W - 1.0) / W, W, dtype=dtype)
    ey = (hm.sum(3) * vy).sum(-1)
    ex = (hm.sum(2) * vx).sum(-1)
    return hm, torch.stack([ex, ey], -1).view(B, K, 2)


def softargmax_bwd(z, dpts, dhm, dtype):
    """d(sum pts dpts + sum hm dhm)/dz [B,K,H,W] by autograd in `dtype`, returned as float64; dpts / dhm may be None"""
    zz = z.detach().to(dtype).clone().requires_grad_(True)
    hm, pts = softargmax(zz, dtype)
    obj = zz.sum() * 0
    if dpts is not None:
        obj = obj + (pts * dpts.to(dtype)).sum()
    if dhm is not None:
        obj = obj + (hm * dhm.to(dtype)).sum()
    obj.backward()
    return zz.grad.double()


def cross_ratio(hm, pts, thm, tpts, loss_type, geo, gamma_h, gamma_v, gscale, dtype, want_grad=True):
    """-> out3 [3] = (location, geo, total), dpts [B,7,2] (or None), float64 tensors of the values computed in `dtype`.
    gscale = (upstream gradient of the location part, of the geo part) or None for ones; out3 is not scaled by it."""
    c = lambda t: None if t is None else t.detach().to(dtype)      # noqa: E731
    p = c(pts).clone().requires_grad_(want_grad)
    loc, gl, tot = ro.cross_ratio_loss(c(hm), p, c(thm), c(tpts), loss_type, geo, gamma_h, gamma_v)
    gl = torch.as_tensor(gl, dtype=dtype)
    out3 = torch.stack([loc.detach().double(), gl.detach().double(), (loc + gl).detach().double()])
    if not want_grad:
        return out3, None
    up = (1.0, 1.0) if gscale is None else gscale
    obj = up[0] * loc + up[1] * gl
    if obj.requires_grad:
        obj.backward()
    return out3, (p.grad if p.grad is not None else torch.zeros_like(p)).double()
