"""Plain torch-CPU references of the layout, weight-pack, max-pool and nearest-upsample kernels (csrc/layout.hip, pack_weights.hip,
pool_upsample.hip) for tests/test_gpu_datamove.py.  No GPU, no torch.nn.functional: slices, comparisons and short sums only.
tests/test_datamove_refs.py pins every function here to torch.nn.functional with autograd.

Activations are NCHW tensors whose values are already numbers of the element type; device buffers are NHWC.  bf16 values are rounded to
nearest even through torch.bfloat16 on the CPU.  All of these operations are exact (copies, maxima, sums of a few integers), so the device
test compares bit patterns; `bits` maps every NaN to one pattern first, because no side promises a NaN's sign or payload.

Max-pool: scan the window in (kh, kw) order with torch's update rule `v > best || isnan(v)`, starting from best = -inf, idx = 0.  So the
first maximum wins, a NaN beats everything but a later NaN, and a window of only -inf keeps idx = 0 -- whatever sits at position 0, even
padding.  There torch points at the first element inside the image instead; nothing here or on the device follows that."""
import torch

F32, BF16 = 0, 1
TD = {F32: torch.float32, BF16: torch.bfloat16}
NONE = 255                                                   # an idx value that no window position equals (k <= 15: positions <= 224)


def rnd(t, dt):
    """the values of `t` as numbers of the element type, held in float32"""
    return t.to(TD[dt]).float()


def bits(t):
    """bit patterns as integers, every NaN mapped to the quiet NaN 0x7FC0 / 0x7FC00000"""
    wide = t.element_size() == 4
    v = t.contiguous().view(torch.int32 if wide else torch.int16)
    return torch.where(torch.isnan(t.contiguous()), torch.full_like(v, 0x7FC00000 if wide else 0x7FC0), v)


# ---------------------------------------------------------------- layout

def nhwc_of(x_nchw, Cpad, dt):
    """[B, C, H, W] -> [B, H, W, Cpad] of the element type, pad channels +0"""
    B, C, H, W = x_nchw.shape
    out = torch.zeros(B, H, W, Cpad, dtype=TD[dt])
    out[..., :C] = x_nchw.permute(0, 2, 3, 1).to(TD[dt])
    return out


def nchw_of(buf, C):
    """[B, H, W, >= C] of any element type -> [B, C, H, W] float32"""
    return buf[..., :C].permute(0, 3, 1, 2).float().contiguous()


# ---------------------------------------------------------------- weight pack

def pack_ref(w_oihw, cout_pad, cin_pad, dt):
    """OIHW fp32 -> wf[n][tap][ci] (n < cout_pad) and wd[ci][tap][co] (ci < cin_pad), tap = kh * KW + kw, padding +0"""
    Co, Ci, KH, KW = w_oihw.shape
    w = w_oihw.reshape(Co, Ci, KH * KW).to(TD[dt])
    wf = torch.zeros(cout_pad, KH * KW, cin_pad, dtype=TD[dt])
    wd = torch.zeros(cin_pad, KH * KW, cout_pad, dtype=TD[dt])
    wf[:Co, :, :Ci] = w.permute(0, 2, 1)
    wd[:Ci, :, :Co] = w.permute(1, 2, 0)
    return wf, wd


# ---------------------------------------------------------------- max-pool

def pool_out(n, k, s, pad):
    return (n + 2 * pad - k) // s + 1


def _scan(xp, inside, k, s, Ho, Wo, pad_pos, last_max=False):
    """xp: the padded input, inside: [Hp, Wp] bool, True on real pixels; a padding position that wins is recorded as pad_pos"""
    B, C = xp.shape[:2]
    best = torch.full((B, C, Ho, Wo), float("-inf"))
    idx = torch.zeros(B, C, Ho, Wo, dtype=torch.uint8)
    for kh in range(k):
        for kw in range(k):
            hs, ws = slice(kh, kh + (Ho - 1) * s + 1, s), slice(kw, kw + (Wo - 1) * s + 1, s)
            v = xp[:, :, hs, ws]
            upd = (v >= best if last_max else v > best) | torch.isnan(v)
            pos = torch.where(inside[hs, ws], kh * k + kw, pad_pos).to(torch.uint8)
            best = torch.where(upd, v, best)
            idx = torch.where(upd, pos.expand_as(idx), idx)
    return best, idx


def _padded(x, lo, hi, value):
    B, C, H, W = x.shape
    xp = torch.full((B, C, H + lo + hi, W + lo + hi), value, dtype=x.dtype)
    xp[:, :, lo:lo + H, lo:lo + W] = x
    inside = torch.zeros(H + lo + hi, W + lo + hi, dtype=torch.bool)
    inside[lo:lo + H, lo:lo + W] = True
    return xp, inside


def maxpool2x2_ref(x, stride, last_max=False):
    """stride 2: floor(H / 2) x floor(W / 2) windows, the odd last row / column belongs to none.  stride 1: H x W windows on the input padded
    with one row / column of zeros at the bottom / right; the zero takes part in the maximum and idx = 4 where it wins."""
    B, C, H, W = x.shape
    if stride == 2:
        xp, inside = _padded(x, 0, 0, 0.0)
        return _scan(xp, inside, 2, 2, H // 2, W // 2, 4, last_max)
    xp, inside = _padded(x, 0, 1, 0.0)
    return _scan(xp, inside, 2, 1, H, W, 4, last_max)


def maxpool_ref(x, k, s, pad, last_max=False):
    """nn.MaxPool2d(k, s, pad): padding is -inf and never wins, so its positions never enter idx -- except as the untouched idx = 0"""
    B, C, H, W = x.shape
    xp, inside = _padded(x, pad, pad, float("-inf"))
    return _scan(xp, inside, k, s, pool_out(H, k, s, pad), pool_out(W, k, s, pad), 0, last_max)


def maxpool_bwd_ref(dy, idx, H, W, k, s, pad):
    """dx[pixel] = sum of dy over the windows that contain the pixel and whose idx names it; float64.  What names a padding position, 4 or
    any other value goes nowhere.  (2x2 forms: k = 2, pad = 0; stride 1 pads at the bottom / right only, which the crop below takes care of.)"""
    B, C, Ho, Wo = dy.shape
    Hp, Wp = max(H + 2 * pad, (Ho - 1) * s + k), max(W + 2 * pad, (Wo - 1) * s + k)
    dxp = torch.zeros(B, C, Hp, Wp, dtype=torch.float64)
    for kh in range(k):
        for kw in range(k):
            dxp[:, :, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s] += dy.double() * (idx == kh * k + kw)
    return dxp[:, :, pad:pad + H, pad:pad + W].contiguous()


# ---------------------------------------------------------------- nearest upsample

def upsample_ref(x, sc):
    return x.repeat_interleave(sc, 2).repeat_interleave(sc, 3)


def upsample_bwd_ref(dy, sc):
    B, C, Hs, Ws = dy.shape
    return dy.double().reshape(B, C, Hs // sc, sc, Ws // sc, sc).sum((3, 5))
