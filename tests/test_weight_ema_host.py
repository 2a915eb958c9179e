"""The weight EMA's host side and its NumPy restatement (tests/weight_ema_ref.py), without a GPU: the C interface, the decay schedule's
properties, the skip, the swap, WeightEMA's argument checks and the training script's two flags."""
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import weight_ema_ref as R
from mdcv import _lib

f32 = np.float32
ENTRY_POINTS = ("mdcv_ema_advance", "mdcv_ema_update", "mdcv_ema_update_segments", "mdcv_ema_swap", "mdcv_ema_swap_segments")


def test_header_declares_the_entry_points_and_the_blocks():
    protos = _lib.parse_header()
    for name in ENTRY_POINTS:
        assert name in protos, name
    assert protos["mdcv_ema_advance"][2] == ["block", "guard", "decay", "warmup", "stream"]
    assert protos["mdcv_ema_update"][2] == ["ema", "params", "n", "block", "stream"]
    assert protos["mdcv_ema_update_segments"][2] == ["ema", "ema_elems", "table", "n_segments", "block", "stream"]
    assert protos["mdcv_ema_swap"][2] == ["ema", "params", "n", "stream"]
    # the optimizer entry points keep their signatures
    assert protos["mdcv_adam_step"][2][-2:] == ["grad_scale", "stream"] and protos["mdcv_adam_step_guarded"][2][5] == "block"
    from mdcv import optim
    text = open(_lib.HEADER).read()
    assert int(re.search(r"#define MDCV_EMA_THREADS (\d+)", text).group(1)) == R.THREADS
    assert int(re.search(r"#define MDCV_EMA_MAX_GRID (\d+)", text).group(1)) == R.MAX_GRID
    assert R.PASS < 4 * 1024 * 1024
    size = {"double": 8, "float": 4, "int": 4, "long long": 8, "const float*": 8}
    for struct, want in (("mdcv_ema_block", 8 * optim._EMA_BLOCK_WORDS), ("mdcv_ema_segment", 24)):
        body = re.search(r"typedef struct %s \{(.*?)\}" % struct, text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        total = sum(size[m.group(1)] * (m.group(2).count(",") + 1)
                    for m in re.finditer(r"(const float\*|double|float|int|long long)\s+([\w\s,]+);", body))
        assert total == want, (struct, total)


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.9, 0.9999])
def test_warmup_one_is_a_constant_decay(decay):
    for t in list(range(50)) + [10 ** 3, 10 ** 6, 2 ** 40]:
        d = R.decay_at(decay, 1, t)
        assert d.dtype == np.float32 and d == f32(decay)


@pytest.mark.parametrize("decay,warmup,strict", [(0.9, 10, True), (0.5, 3, True), (0.99, 2000, False), (0.9999, 10, False), (0.0, 7, True)], ids=str)
def test_schedule_is_non_decreasing_and_reaches_the_decay_where_the_rule_says(decay, warmup, strict):
    dd = Fraction(float(f32(decay)))                         # the decay as the kernel sees it
    # (1 + t) / (warmup + t) >= dd  <=>  t >= (dd * warmup - 1) / (1 - dd), in exact arithmetic
    q = (dd * warmup - 1) / (1 - dd)
    t_reach = max(0, -((-q.numerator) // q.denominator))
    assert Fraction(1 + t_reach, warmup + t_reach) >= dd and (t_reach == 0 or Fraction(t_reach, warmup + t_reach - 1) < dd)
    ts = sorted(set(list(range(0, 200)) + list(range(max(0, t_reach - 50), t_reach + 50)) + [t_reach * 3 + 7, 10 ** 7]))
    ds = [R.decay_at(decay, warmup, t) for t in ts]
    assert all(a <= b for a, b in zip(ds, ds[1:]))
    assert all(0.0 <= d <= f32(decay) for d in ds)
    assert all(d == f32(decay) for t, d in zip(ts, ds) if t >= t_reach)
    # strict: the ramp's step at t_reach, (warmup - 1) / (warmup + t)^2, is far larger than an fp32 ulp (6e-8), so no earlier t rounds up to the
    # decay; where it is not (0.99 / 2000: 5e-8, 0.9999 / 10: 1e-9) a few earlier updates may already round to it
    if strict and t_reach > 0:
        assert all(d < f32(decay) for t, d in zip(ts, ds) if t < t_reach)
    if warmup > 1 and t_reach > 0:
        assert ds[0] == f32(np.float64(1.0) / np.float64(warmup))


def test_restated_sequence_update_skip_and_swap():
    rng = np.random.default_rng(0)
    e = rng.standard_normal(37).astype(np.float32)
    blk = R.new_block()
    for t in range(5):
        p = rng.standard_normal(37).astype(np.float32)
        before = e.copy()
        R.advance(blk, 0.9, 10)
        assert blk["updates"] == t + 1 and blk["apply"] == 1 and blk["d"] == R.decay_at(0.9, 10, t) and blk["omd"] == f32(1) - blk["d"]
        R.update(blk, e, p)
        # three roundings, by hand
        want = before + (blk["omd"] * (p - before).astype(np.float32)).astype(np.float32)
        assert e.dtype == np.float32 and np.array_equal(e.view(np.uint32), want.astype(np.float32).view(np.uint32))
    # a skipped advance changes nothing but the flag, and the update behind it nothing at all
    snap, eb = dict(blk), e.copy()
    R.advance(blk, 0.9, 10, guard_apply=0)
    R.update(blk, e, rng.standard_normal(37).astype(np.float32))
    assert blk == dict(snap, apply=0) and np.array_equal(e.view(np.uint32), eb.view(np.uint32))
    R.advance(blk, 0.9, 10, guard_apply=1)
    assert blk["updates"] == 6 and blk["d"] == R.decay_at(0.9, 10, 5)
    # the first update with warmup 1 and decay 0 copies p (e + (p - e) is p wherever the difference is exact)
    z = np.zeros(4, np.float32)
    R.update(R.advance(R.new_block(), 0.0, 1), z, np.array([1, -2, 0.5, 0], np.float32))
    assert z.tolist() == [1.0, -2.0, 0.5, 0.0]
    # swap: an involution on the bits, NaN payloads and signed zeros included
    a = np.array([0x7fc00001, 0x80000000, 1, 0x3f800000], np.uint32).view(np.float32).copy()
    b = np.array([0xffc12345, 0, 0x80000001, 0xbf800000], np.uint32).view(np.float32).copy()
    a0, b0 = a.view(np.uint32).copy(), b.view(np.uint32).copy()
    R.swap(a, b)
    assert np.array_equal(a.view(np.uint32), b0) and np.array_equal(b.view(np.uint32), a0)
    R.swap(a, b)
    assert np.array_equal(a.view(np.uint32), a0) and np.array_equal(b.view(np.uint32), b0)


def test_the_package_restates_the_decay_rule_for_its_log_line():
    from mdcv.optim import ema_decay_at
    for decay, warmup in ((0.9, 10), (0.9999, 10), (0.5, 1)):
        for t in (0, 1, 9, 80, 81, 10 ** 5):
            assert ema_decay_at(decay, warmup, t) == float(R.decay_at(decay, warmup, t))


def test_weight_ema_checks_its_arguments():
    from mdcv.optim import FusedAdam, WeightEMA
    from mdcv.rektnet.keypoint_net import KeypointNet
    net = KeypointNet(7, (80, 80))
    with pytest.raises(TypeError):
        WeightEMA(list(net.parameters()))
    with pytest.raises(TypeError):
        WeightEMA(torch.nn.Linear(2, 2))
    for bad in (-0.1, 1.0, 1.5, float("nan"), 0.99999999, "0.9", None, True):     # 0.99999999 rounds to 1.0f
        with pytest.raises(ValueError):
            WeightEMA(net, decay=bad)
    for bad in (0, -3, 2.5, "10", None, True):
        with pytest.raises(ValueError):
            WeightEMA(net, warmup=bad)
    ema = WeightEMA(net)                                     # a model still on the host: nothing is allocated, nothing has happened
    assert (ema.decay, ema.warmup, ema.updates) == (0.9999, 10, 0) and ema.block()["updates"] == 0
    assert WeightEMA(net, decay=0, warmup=1).decay == 0.0
    with pytest.raises(TypeError):
        FusedAdam(net, ema=object())
    with pytest.raises(ValueError):
        FusedAdam(net, ema=WeightEMA(KeypointNet(7, (80, 80))))
    assert FusedAdam(net, ema=ema).ema is ema and FusedAdam(net).ema is None
    assert "ema" not in FusedAdam(net).state_dict()


def test_parser_takes_the_two_flags_and_their_defaults_mean_off(monkeypatch):
    from mdcv.yolo import train as yt
    opt = yt._parser().parse_args(["--model_cfg", "mini.cfg"])
    assert opt.ema_decay == 0.0 and opt.ema_warmup == 10
    opt = yt._parser().parse_args(["--model_cfg", "mini.cfg", "--ema_decay", "0.999", "--ema_warmup", "25"])
    assert opt.ema_decay == 0.999 and opt.ema_warmup == 25
    seen = {}
    monkeypatch.setattr(yt, "train", lambda **kw: seen.update(kw))
    yt.main(["--model_cfg", "mini.cfg"])
    assert seen["ema_decay"] == 0.0 and seen["ema_warmup"] == 10
    yt.main(["--model_cfg", "mini.cfg", "--ema_decay", "0.9", "--ema_warmup", "3"])
    assert seen["ema_decay"] == 0.9 and seen["ema_warmup"] == 3
