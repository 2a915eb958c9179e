"""NumPy restatement of csrc/weight_ema.hip, operation for operation (include/mdcv_hip.h): the decay rule in fp64 rounded once
to fp32, the update as a subtraction, a product and a sum that each round to fp32 on their own -- what the kernels do, built without fma
contraction -- the skip of an update the gradient guard dropped, and the swap.  The GPU tests compare with `==`."""
import numpy as np

THREADS = 256         # MDCV_EMA_THREADS
MAX_GRID = 2048       # MDCV_EMA_MAX_GRID
PASS = MAX_GRID * THREADS * 4          # elements one grid pass of the range kernels covers
f32 = np.float32


def new_block():
    """mdcv_ema_block after the caller zeroed it"""
    return dict(updates=0, d=f32(0.0), omd=f32(0.0), apply=0)


def decay_at(decay, warmup, t):
    """d of update number t (0-based): min((double)(float)decay, (1 + t) / (warmup + t)) in fp64, then rounded to fp32"""
    d64 = min(np.float64(f32(decay)), (np.float64(1.0) + np.float64(t)) / (np.float64(warmup) + np.float64(t)))
    return f32(d64)


def advance(blk, decay, warmup, guard_apply=None):
    """mdcv_ema_advance: guard_apply None (no guard) or the guard block's `apply`"""
    if guard_apply is not None and int(guard_apply) == 0:
        blk["apply"] = 0
        return blk
    t = blk["updates"]
    d = decay_at(decay, warmup, t)
    blk["d"], blk["omd"], blk["apply"], blk["updates"] = d, f32(f32(1.0) - d), 1, t + 1
    return blk


def update(blk, e, p):
    """mdcv_ema_update / _segments in place on the fp32 array e: e + omd * (p - e), three roundings; apply == 0: nothing"""
    if blk["apply"] == 0:
        return e
    p = np.asarray(p, np.float32)
    with np.errstate(all="ignore"):
        diff = (p - e).astype(np.float32)
        step = (blk["omd"] * diff).astype(np.float32)
        e[...] = (e + step).astype(np.float32)
    return e


def swap(e, p):
    """mdcv_ema_swap: the two arrays exchange their 32-bit words"""
    a, b = e.view(np.uint32), p.view(np.uint32)
    t = a.copy()
    a[...] = b
    b[...] = t
