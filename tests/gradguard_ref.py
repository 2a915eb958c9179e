"""NumPy restatement of csrc/grad_guard.hip, operation for operation (include/mdcv_hip.h): the chunked fp64 sum of squares, the
finalize step's control block, and the guarded Adam / SGD updates in fp32 with every product, sum, quotient and root rounded on its own --
which is what the kernels do, built without fma contraction.  The GPU tests compare with `==`."""
import numpy as np

CHUNK = 4096          # MDCV_GRAD_GUARD_CHUNK
MAX_GRID = 2048       # MDCV_GRAD_GUARD_MAX_GRID
_LANE = np.arange(64)
f32 = np.float32


def block_sum_256(acc):
    """[k, 256] float64 -> [k]: the xor butterfly of each 64-lane wave (offsets 32 .. 1), then ((w0 + w1) + w2) + w3"""
    v = np.asarray(acc, np.float64).reshape(-1, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, _LANE ^ o]
    w = v[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def sumsq_partials(g):
    """one fp64 partial per chunk of 4096 elements of the fp32 vector g: thread t adds elements (r * 256 + t) * 4 + e, r then e ascending"""
    g = np.asarray(g, np.float32).reshape(-1)
    n = g.size
    nch = (n + CHUNK - 1) // CHUNK
    x = np.zeros(nch * CHUNK, np.float64)
    x[:n] = g.astype(np.float64)
    with np.errstate(all="ignore"):
        sq = (x * x).reshape(nch, 4, 256, 4)
        acc = np.zeros((nch, 256), np.float64)
        for r in range(4):
            for e in range(4):
                acc = acc + sq[:, r, :, e]
        return block_sum_256(acc)


def sum_partials(partials):
    """thread t adds partials t, t + 256, .. in order; then block_sum_256"""
    p = np.asarray(partials, np.float64)
    rows = (p.size + 255) // 256
    x = np.zeros(rows * 256, np.float64)
    x[:p.size] = p
    x = x.reshape(rows, 256)
    with np.errstate(all="ignore"):
        acc = np.zeros(256, np.float64)
        for r in range(rows):
            acc = acc + x[r]
        return block_sum_256(acc[None])[0]


def sumsq(g):
    return sum_partials(sumsq_partials(g))


def pow_d(beta, t):
    """beta ** t by square-and-multiply from the low bit of t up, every product one IEEE double rounding"""
    r, x, t = np.float64(1.0), np.float64(beta), int(t)
    with np.errstate(all="ignore"):
        while t > 0:
            if t & 1:
                r = r * x
            t >>= 1
            if t > 0:
                x = x * x
    return r


def bias_corrections(beta1, beta2, t):
    """(bc1, bc2_sqrt) as the finalize step stores them: one rounding to fp32 of a double expression"""
    return f32(np.float64(1.0) - pow_d(beta1, t)), f32(np.sqrt(np.float64(1.0) - pow_d(beta2, t)))


def clip_coef(norm, max_norm):
    """fminf(1, max_norm / (norm + 1e-6f)) in fp32 (fminf returns the number when the other argument is NaN); max_norm <= 0: 1"""
    if not max_norm > 0:
        return f32(1.0)
    with np.errstate(all="ignore"):
        return np.fmin(f32(1.0), f32(max_norm) / (f32(norm) + f32(1e-6)))


def new_block():
    return dict(sumsq=0.0, norm=f32(0), coef=f32(0), scale=f32(0), bc1=f32(0), bc2_sqrt=f32(0), max_norm=f32(0), finite=0, apply=0,
                attempted=0, applied=0, skipped=0, clipped=0, norms=[])


def finalize(blk, g, grad_scale=1.0, max_norm=0.0, skip_nonfinite=True, beta1=0.0, beta2=0.0, ring=1024):
    """mdcv_grad_guard_finalize over the gradient g on the block `blk` (a dict as GradGuard.stats() returns, updated in place);
    beta1 / beta2 are the fp32-rounded values the update kernels use, widened to double"""
    gs = f32(grad_scale)
    s = sumsq(g)
    finite = int(np.isfinite(s))
    with np.errstate(all="ignore"):
        norm = f32(np.abs(np.float64(gs)) * np.sqrt(s))
        coef = clip_coef(norm, max_norm)
        scale = gs * coef
    apply = int(bool(finite) or not skip_nonfinite)
    t = blk["applied"] + 1
    bc1, bc2_sqrt = bias_corrections(np.float64(f32(beta1)), np.float64(f32(beta2)), t)
    blk.update(sumsq=float(s), norm=norm, coef=coef, scale=scale, bc1=bc1, bc2_sqrt=bc2_sqrt, finite=finite, apply=apply)
    if finite and norm > blk["max_norm"]:
        blk["max_norm"] = norm
    blk["attempted"] += 1
    if apply:
        blk["applied"] += 1
    else:
        blk["skipped"] += 1
    if apply and finite and coef < f32(1.0):
        blk["clipped"] += 1
    blk["norms"] = (blk["norms"] + [norm])[-ring:]
    return blk


def adam_step(blk, p, g, m, v, lr, beta1, beta2, eps, weight_decay):
    """adam_guarded_kernel on fp32 arrays, in place, in the kernel's expression order; nothing happens when blk['apply'] == 0"""
    if not blk["apply"]:
        return
    lr, b1, b2, eps, wd = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(weight_decay)
    gs, bc1, bc2s = f32(blk["scale"]), f32(blk["bc1"]), f32(blk["bc2_sqrt"])
    one = f32(1.0)
    with np.errstate(all="ignore"):
        gr = g * gs + wd * p
        m[:] = b1 * m + (one - b1) * gr
        v[:] = b2 * v + ((one - b2) * gr) * gr
        p[:] = p - ((lr / bc1) * m) / (np.sqrt(v) / bc2s + eps)


def sgd_step(blk, p, g, buf, lr, momentum, weight_decay):
    """sgd_guarded_kernel; the first APPLIED step initialises the momentum buffer with the gradient"""
    if not blk["apply"]:
        return
    lr, mo, wd, gs = f32(lr), f32(momentum), f32(weight_decay), f32(blk["scale"])
    with np.errstate(all="ignore"):
        gr = g * gs + wd * p
        if mo != 0:
            b = gr if blk["applied"] == 1 else mo * buf + gr
            buf[:] = b
            gr = b
        p[:] = p - lr * gr
