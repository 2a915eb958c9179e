"""The gradient guard's host side and its NumPy restatement (tests/gradguard_ref.py), without a GPU: the C interface, the error of the
restated sum against the exact sum, the bias corrections against Python's doubles, the clip coefficient against torch's clip_grad_norm_."""
import math
import re

import numpy as np
import pytest
import torch

import gradguard_ref as R
from mdcv import _lib

ENTRY_POINTS = ("mdcv_grad_sumsq", "mdcv_grad_guard_finalize", "mdcv_adam_step_guarded", "mdcv_sgd_step_guarded")


def test_header_declares_the_entry_points_and_the_package_exports_the_guard():
    protos = _lib.parse_header()
    for name in ENTRY_POINTS:
        assert name in protos, name
    assert protos["mdcv_grad_sumsq"][2] == ["grads", "n", "partials", "stream"]
    assert protos["mdcv_adam_step_guarded"][2][:6] == ["params", "grads", "exp_avg", "exp_avg_sq", "n", "block"]
    assert protos["mdcv_sgd_step_guarded"][2][:5] == ["params", "grads", "momentum_buf", "n", "block"]
    # the unguarded entry points keep their signatures
    assert protos["mdcv_adam_step"][2][-2:] == ["grad_scale", "stream"] and protos["mdcv_sgd_step"][2][-2:] == ["grad_scale", "stream"]
    from mdcv import optim
    from mdcv.optim import GradGuard, grad_norm            # noqa: F401
    text = open(_lib.HEADER).read()
    assert int(re.search(r"#define MDCV_GRAD_GUARD_CHUNK (\d+)", text).group(1)) == optim.GUARD_CHUNK == R.CHUNK
    assert int(re.search(r"#define MDCV_GRAD_GUARD_MAX_GRID (\d+)", text).group(1)) == R.MAX_GRID
    # the block the Python side reads as 9 int64 words: 72 bytes by the struct's own fields
    body = re.search(r"typedef struct mdcv_grad_guard_block \{(.*?)\}", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"double": 8, "float": 4, "int": 4, "long long": 8}
    total = sum(size[m.group(1)] * (m.group(2).count(",") + 1) for m in re.finditer(r"(double|float|int|long long)\s+([\w\s,]+);", body))
    assert total == 72 == 8 * optim._BLOCK_WORDS


def test_guard_arguments_and_idle_state():
    from mdcv.optim import GradGuard
    g = GradGuard()
    assert g.max_norm == 0.0 and g.skip_nonfinite is True and g.ring == 1024
    assert GradGuard(max_norm=0).max_norm == 0.0 and GradGuard(max_norm=10).max_norm == 10.0
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            GradGuard(max_norm=bad)
    with pytest.raises(ValueError):
        GradGuard(ring=0)
    s = g.stats()                                           # nothing measured: no device is touched
    assert s["attempted"] == s["applied"] == s["skipped"] == s["clipped"] == 0 and s["norms"] == []
    g.load_state_dict(dict(attempted=7, applied=5, skipped=2, clipped=1, max_norm=3.5))
    assert g.state_dict() == dict(attempted=7, applied=5, skipped=2, clipped=1, max_norm=3.5)
    with pytest.raises(RuntimeError):
        g.norm


def _wide_gradients(n, seed):
    """fp32 values from the smallest denormal to 3e38, both signs"""
    rng = np.random.default_rng(seed)
    g = np.clip(rng.standard_normal(n) * 10.0 ** rng.uniform(-44, 38, n), -3e38, 3e38).astype(np.float32)
    fixed = np.array([1e-45, -1e-45, 1.1754942e-38, 3e38, -3e38, 0.0, 1.0], np.float32)
    k = min(n, fixed.size)
    g[:k] = fixed[:k]
    return g


@pytest.mark.parametrize("n", [1, 3, 255, 4097, 100003])
def test_restated_sum_is_within_the_bound_of_any_summation_order(n):
    """Every term is >= 0, so n - 1 additions in ANY order are within (n - 1) 2^-53 of the exact sum, relatively; the squares are exact."""
    g = _wide_gradients(n, n)
    exact_sq = [float(x) * float(x) for x in g.astype(np.float64)]
    assert all(float(np.float64(x) * np.float64(x)) == e for x, e in zip(g[:64].astype(np.float64), exact_sq[:64]))
    want = math.fsum(exact_sq)
    assert math.isfinite(want) and want > 0
    got = float(R.sumsq(g))
    assert abs(got - want) <= (n - 1) * 2.0 ** -53 * want, (got, want)
    # one partial per chunk, each the sum of its own elements
    parts = R.sumsq_partials(g)
    assert parts.size == (n + R.CHUNK - 1) // R.CHUNK
    for c in (0, parts.size - 1):
        w = math.fsum(exact_sq[c * R.CHUNK:(c + 1) * R.CHUNK])
        assert abs(float(parts[c]) - w) <= (R.CHUNK - 1) * 2.0 ** -53 * w


def test_restated_sum_flags_every_non_finite_gradient():
    for bad in (np.nan, np.inf, -np.inf):
        for pos in (0, 4092, 4096):
            g = np.ones(4097, np.float32)
            g[pos] = bad
            assert not np.isfinite(R.sumsq(g))
    big = float(R.sumsq(np.full(4097, 3e38, np.float32)))                                            # no overflow in double
    assert math.isfinite(big) and abs(big - 4097 * float(np.float32(3e38)) ** 2) <= 4097 * 2.0 ** -53 * big
    assert R.sumsq(np.zeros(5, np.float32)) == 0.0


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("beta", [0.9, 0.999])
@pytest.mark.parametrize("t", [1, 2, 3, 1000, 8388608])
def test_bias_corrections_within_one_ulp_of_the_correctly_rounded_value(beta, t):
    """The inputs are doubles and the stored value is rounded to fp32 once: within one fp32 ulp of round(1 - beta ** t)."""
    bc1, bc2s = R.bias_corrections(beta, beta, t)
    want1 = np.float32(1 - beta ** t)
    want2 = np.float32(math.sqrt(1 - beta ** t))
    assert bc1.dtype == np.float32 and bc2s.dtype == np.float32
    assert abs(float(bc1) - float(want1)) <= _ulp32(want1), (float(bc1), float(want1))
    assert abs(float(bc2s) - float(want2)) <= _ulp32(want2), (float(bc2s), float(want2))
    if t == 1:
        assert float(R.pow_d(beta, 1)) == beta
    assert 0.0 < float(bc1) <= 1.0


def test_pow_d_is_the_documented_product_chain():
    b = np.float64(np.float32(0.999))
    assert R.pow_d(b, 2) == b * b and R.pow_d(b, 3) == b * (b * b) and R.pow_d(b, 5) == b * ((b * b) * (b * b))
    assert R.pow_d(b, 0) == 1.0 and R.pow_d(0.0, 7) == 0.0


@pytest.mark.parametrize("scale,max_norm", [(1.0, 1.0), (100.0, 10.0), (1e-3, 10.0), (1.0, 1e4)])
def test_clip_coefficient_against_torch_clip_grad_norm(scale, max_norm):
    """torch adds up in fp32 (a norm per tensor, then the norm of those), the guard in fp64: the coefficients agree as far as torch's norm
    agrees with the fp64 norm of the same gradients, which is measured here, plus the three fp32 roundings of the coefficient itself
    (the cast of the norm, the sum with 1e-6, the quotient) on either side."""
    gen = torch.Generator().manual_seed(11)
    shapes = [(64, 3, 3, 3), (64,), (255, 128), (200003,), (5,)]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen) * scale
    flat = np.concatenate([p.grad.numpy().reshape(-1) for p in params])
    before = [p.grad.clone() for p in params]
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    norm64 = math.sqrt(math.fsum(float(x) * float(x) for x in flat.astype(np.float64)))
    torch_dev = abs(float(total) - norm64) / norm64
    print(f"torch fp32 norm {float(total)!r} vs fp64 {norm64!r}: relative deviation {torch_dev:.3e}")
    blk = R.finalize(R.new_block(), flat, 1.0, max_norm)
    assert abs(float(blk["norm"]) - norm64) <= 2.0 ** -24 * norm64                # fp64 sum, one rounding to fp32
    torch_coef = float(torch.clamp(max_norm / (total + 1e-6), max=1.0))
    tol = torch_dev + 3 * 2.0 ** -24
    assert abs(float(blk["coef"]) - torch_coef) <= tol * torch_coef, (float(blk["coef"]), torch_coef, tol)
    assert (float(blk["coef"]) < 1.0) == (norm64 > max_norm) and blk["clipped"] == int(norm64 > max_norm)
    # and the gradients torch left behind are the originals times that coefficient, to the same tolerance (one more rounding)
    k = 3
    got, want = params[k].grad.double(), before[k].double() * float(blk["coef"])
    assert float((got - want).abs().max()) <= (tol + 2.0 ** -24) * float(want.abs().max())


def test_finalize_restatement_counts_and_skips():
    blk = R.new_block()
    g = np.ones(10, np.float32)
    R.finalize(blk, g, 1.0, 0.0, True, 0.9, 0.999)
    assert (blk["attempted"], blk["applied"], blk["skipped"], blk["apply"], float(blk["coef"])) == (1, 1, 0, 1, 1.0)
    bad = g.copy()
    bad[3] = np.nan
    first = (blk["bc1"], blk["bc2_sqrt"])
    R.finalize(blk, bad, 1.0, 0.0, True, 0.9, 0.999)
    assert (blk["attempted"], blk["applied"], blk["skipped"], blk["apply"], blk["finite"]) == (2, 1, 1, 0, 0)
    R.finalize(blk, g, 1.0, 0.0, True, 0.9, 0.999)
    second = R.bias_corrections(np.float64(np.float32(0.9)), np.float64(np.float32(0.999)), 2)
    assert (blk["bc1"], blk["bc2_sqrt"]) == second != first and blk["applied"] == 2          # t = applied + 1, not attempted
    R.finalize(blk, bad, 1.0, 0.0, False, 0.9, 0.999)
    assert blk["apply"] == 1 and blk["finite"] == 0 and blk["applied"] == 3 and blk["clipped"] == 0
    assert float(blk["max_norm"]) == float(np.float32(math.sqrt(10.0)))
