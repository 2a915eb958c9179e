"""-m gpu: the weight EMA (csrc/weight_ema.hip, mdcv.optim.WeightEMA) against its NumPy restatement (tests/weight_ema_ref.py), as bits: the
range update and the swap on aligned sub-ranges between sentinels, the segment-table form on sources at odd offsets, the advance over a
sequence with skipped steps, a mini Darknet under FusedAdam (plain, pipelined, guarded with a poisoned step), `applied()`, the state
dicts, and the two training loops."""
import contextlib
import functools
import io
import os
import shutil

import numpy as np
import pytest
import torch

import weight_ema_ref as R

pytestmark = pytest.mark.gpu

from mdcv import _lib  # noqa: E402
from mdcv.optim import FusedAdam, GradGuard, WeightEMA  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MINI = os.path.join(G, "mini")
f32 = np.float32


def st():
    return torch.cuda.current_stream().cuda_stream


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(t, a):
    """device fp32 tensor == NumPy fp32 array, bit for bit (signed zeros and denormals included)"""
    got, want = t.detach().cpu().numpy(), np.asarray(a, np.float32)
    nan = np.isnan(want)                 # (a NaN a host operation CREATES carries the host's sign bit: NaNs are compared as NaNs)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def wide(n, seed, kind="wide"):
    """tests/test_gpu_gradguard.py's generator: denormals .. 3e38, fixed extremes; here with zeros of both signs as well"""
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros(n, np.float32)
    g = np.clip(rng.standard_normal(n) * 10.0 ** rng.uniform(-44, 38, n), -3e38, 3e38).astype(np.float32)      # denormals .. 3e38
    fixed = np.array([1e-45, -3e38, 3e38, -1e-45, 1.1754942e-38, 0.0, -0.0], np.float32)
    pos = rng.permutation(n)[:fixed.size]
    g[pos] = fixed[:pos.size]
    return g


def read_block(blk):
    w = blk.cpu()
    f, i = w.view(torch.float32), w.view(torch.int32)
    return dict(updates=int(w[0]), d=f32(float(f[2])), omd=f32(float(f[3])), apply=int(i[4]))


def block_equal(got, want):
    return [(k, got[k], want[k]) for k in ("updates", "d", "omd", "apply") if not got[k] == want[k]]


def guard_block(apply):
    """a hand-written mdcv_grad_guard_block: only `apply` (byte 36) matters to the EMA"""
    g = torch.zeros(9, dtype=torch.int64, device="cuda")
    g.view(torch.int32)[9] = int(apply)
    return g


# ---------------------------------------------------------------------------------------------------------------- range update and swap
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, R.PASS + 5]      # the last: more than one pass of the capped grid, and a scalar tail
SENT_E, SENT_P = f32(123.25), f32(-77.5)


@pytest.mark.parametrize("n", SIZES, ids=str)
def test_range_update_and_swap_equal_the_restatement_between_sentinels(n):
    assert n < 4 * 1024 * 1024
    L = _lib.lib()
    for lo in ((4,) if n > 4096 else (4, 20)):                         # 16-byte aligned starts inside a larger buffer: ptr + 4 * lo
        hi_pad = 7
        E, P = wide(n, 2 * n + lo), wide(n, 2 * n + lo + 1)
        E[0], P[0] = (f32(-0.0), f32(0.0)) if n > 1 else (E[0], P[0])
        Eb, Pb = np.full(lo + n + hi_pad, SENT_E, np.float32), np.full(lo + n + hi_pad, SENT_P, np.float32)
        Eb[lo:lo + n], Pb[lo:lo + n] = E, P
        eb, pb = torch.from_numpy(Eb).cuda(), torch.from_numpy(Pb).cuda()
        ep, pp = eb.data_ptr() + 4 * lo, pb.data_ptr() + 4 * lo
        blk = torch.zeros(3, dtype=torch.int64, device="cuda")
        ref = R.new_block()
        for k in range(2):                                              # two updates: omd 0.9, then 1 - 2/11
            L.check(L.ema_advance(blk.data_ptr(), None, 0.9, 10, st()))
            L.check(L.ema_update(ep, pp, n, blk.data_ptr(), st()))
            R.advance(ref, 0.9, 10)
            R.update(ref, Eb[lo:lo + n], P)
            assert block_equal(read_block(blk), ref) == []
            assert same_bits(eb, Eb), (n, lo, k)                        # the range AND the sentinels on both sides
            assert same_bits(pb, Pb)
        # a dropped step: nothing is touched
        L.check(L.ema_advance(blk.data_ptr(), guard_block(0).data_ptr(), 0.9, 10, st()))
        L.check(L.ema_update(ep, pp, n, blk.data_ptr(), st()))
        assert read_block(blk) == dict(ref, apply=0) and same_bits(eb, Eb) and same_bits(pb, Pb)
        # swap: the range's words change sides, the sentinels stay; twice restores every bit
        L.check(L.ema_swap(ep, pp, n, st()))
        Es, Ps = Eb.copy(), Pb.copy()
        R.swap(Es[lo:lo + n], Ps[lo:lo + n])
        assert np.array_equal(u32(Es[lo:lo + n]), u32(P)) and same_bits(eb, Es) and same_bits(pb, Ps)
        L.check(L.ema_swap(ep, pp, n, st()))
        assert same_bits(eb, Eb) and same_bits(pb, Pb)


def test_swap_moves_nan_payloads_unchanged():
    L = _lib.lib()
    a = np.array([0x7fc00001, 0x80000000, 1, 0x3f800000, 0xff800000], np.uint32)
    b = np.array([0xffc12345, 0, 0x80000001, 0xbf800000, 0x7f812345], np.uint32)
    ta, tb = torch.from_numpy(a.view(np.int32).copy()).cuda(), torch.from_numpy(b.view(np.int32).copy()).cuda()
    L.check(L.ema_swap(ta.data_ptr(), tb.data_ptr(), 5, st()))
    assert np.array_equal(ta.cpu().numpy().view(np.uint32), b) and np.array_equal(tb.cpu().numpy().view(np.uint32), a)


def test_bad_arguments_are_refused_before_any_launch():
    L = _lib.lib()
    e, p = torch.ones(64, device="cuda"), torch.zeros(64, device="cuda")
    blk = torch.zeros(3, dtype=torch.int64, device="cuda")
    tab = torch.zeros(3, dtype=torch.int64, device="cuda")
    assert L.ema_advance(None, None, 0.9, 10, st()) == -1 and L.ema_advance(blk.data_ptr(), None, 1.0, 10, st()) == -1
    assert L.ema_advance(blk.data_ptr(), None, -0.1, 10, st()) == -1 and L.ema_advance(blk.data_ptr(), None, 0.9, 0, st()) == -1
    assert L.ema_update(e.data_ptr() + 4, p.data_ptr(), 8, blk.data_ptr(), st()) == -1
    assert L.ema_update(e.data_ptr(), p.data_ptr() + 8, 8, blk.data_ptr(), st()) == -1
    assert L.ema_update(e.data_ptr(), p.data_ptr(), 8, None, st()) == -1 and L.ema_update(e.data_ptr(), p.data_ptr(), -1, blk.data_ptr(), st()) == -1
    assert L.ema_update(None, p.data_ptr(), 8, blk.data_ptr(), st()) == -1
    assert L.ema_update_segments(e.data_ptr(), 64, None, 1, blk.data_ptr(), st()) == -1
    assert L.ema_update_segments(e.data_ptr(), 64, tab.data_ptr(), 1, None, st()) == -1
    assert L.ema_swap(e.data_ptr(), e.data_ptr() + 16, 8, st()) == -1                   # overlapping sides
    assert L.ema_swap(e.data_ptr() + 4, p.data_ptr(), 8, st()) == -1 and L.ema_swap_segments(None, 64, tab.data_ptr(), 1, st()) == -1
    assert L.ema_update(e.data_ptr(), p.data_ptr(), 0, blk.data_ptr(), st()) == 0        # an empty range: nothing to do
    torch.cuda.synchronize()
    assert int(blk.abs().sum()) == 0 and bool((e == 1).all()) and bool((p == 0).all())


# ---------------------------------------------------------------------------------------------------------------- segment table
def test_segment_table_update_and_swap_on_sources_at_odd_offsets():
    L = _lib.lib()
    lengths = [1, 2, 3, 5, 64, 1023, 1024]
    n_flat = 8                                                          # a flat part in front, which the segment launches must not touch
    src_off, sh_off, pos, off = [], [], 1, n_flat
    for ln in lengths:
        src_off.append(pos)                                             # every source starts at an odd element: 4-byte aligned, no more
        pos += ln + (2 if (pos + ln) % 2 == 1 else 1)
        assert pos % 2 == 1
        sh_off.append(off)
        off += (ln + 3) & ~3                                            # shadow segments padded to 4
    total = off
    S = np.full(pos + 3, SENT_P, np.float32)
    E = np.full(total, SENT_E, np.float32)
    for k, (so, eo, ln) in enumerate(zip(src_off, sh_off, lengths)):
        S[so:so + ln], E[eo:eo + ln] = wide(ln, 50 + k), wide(ln, 70 + k)
    src, e = torch.from_numpy(S).cuda(), torch.from_numpy(E).cuda()
    rows = [(src.data_ptr() + 4 * so, eo, ln) for so, eo, ln in zip(src_off, sh_off, lengths)] + [(src.data_ptr(), 3, 0)]   # and an empty row
    tab = torch.tensor(rows, dtype=torch.int64).cuda()
    blk = torch.zeros(3, dtype=torch.int64, device="cuda")
    ref = R.new_block()

    def restate(fn):
        for so, eo, ln in zip(src_off, sh_off, lengths):
            fn(E[eo:eo + ln], S[so:so + ln])
    for k in range(2):
        L.check(L.ema_advance(blk.data_ptr(), guard_block(1).data_ptr(), 0.9, 10, st()))
        L.check(L.ema_update_segments(e.data_ptr(), total, tab.data_ptr(), len(rows), blk.data_ptr(), st()))
        R.advance(ref, 0.9, 10, guard_apply=1)
        restate(lambda ee, ss: R.update(ref, ee, ss))
        assert block_equal(read_block(blk), ref) == [] and same_bits(e, E) and same_bits(src, S)      # pads, flat part, gaps: sentinels still
    L.check(L.ema_advance(blk.data_ptr(), guard_block(0).data_ptr(), 0.9, 10, st()))
    L.check(L.ema_update_segments(e.data_ptr(), total, tab.data_ptr(), len(rows), blk.data_ptr(), st()))
    assert read_block(blk) == dict(ref, apply=0) and same_bits(e, E) and same_bits(src, S)
    E0, S0 = E.copy(), S.copy()
    L.check(L.ema_swap_segments(e.data_ptr(), total, tab.data_ptr(), len(rows), st()))
    restate(R.swap)
    assert same_bits(e, E) and same_bits(src, S) and not np.array_equal(u32(E), u32(E0))
    L.check(L.ema_swap_segments(e.data_ptr(), total, tab.data_ptr(), len(rows), st()))
    assert same_bits(e, E0) and same_bits(src, S0)


# ---------------------------------------------------------------------------------------------------------------- advance
# (0.9, 10) is the case as asked for; its min() switches to the decay at t = 80, behind the sequence's end, so (0.75, 10) -- switch at t = 26 --
# runs as well
@pytest.mark.parametrize("decay,warmup,switch_inside", [(0.9, 10, False), (0.75, 10, True)], ids=str)
def test_advance_sequence_with_skipped_steps_equals_the_restatement(decay, warmup, switch_inside):
    L = _lib.lib()
    n = 1029
    rng = np.random.default_rng(11)
    E = rng.standard_normal(n).astype(np.float32)
    e, p = torch.from_numpy(E.copy()).cuda(), torch.zeros(n, device="cuda")
    blk = torch.zeros(3, dtype=torch.int64, device="cuda")
    ref = R.new_block()
    on, off = guard_block(1), guard_block(0)
    skipped_at = (5, 30)
    ds = []
    for k in range(42):                                                 # 40 updates and two skipped steps
        P = rng.standard_normal(n).astype(np.float32)
        p.copy_(torch.from_numpy(P))
        skip = k in skipped_at
        before_blk, before_e = read_block(blk), e.clone()
        guard = off if skip else (on if k % 2 else None)                # applying: a guard that says so, or none at all
        L.check(L.ema_advance(blk.data_ptr(), None if guard is None else guard.data_ptr(), decay, warmup, st()))
        L.check(L.ema_update(e.data_ptr(), p.data_ptr(), n, blk.data_ptr(), st()))
        R.advance(ref, decay, warmup, guard_apply=0 if skip else None)
        R.update(ref, E, P)
        got = read_block(blk)
        assert block_equal(got, ref) == [] and same_bits(e, E), k
        if skip:
            assert got == dict(before_blk, apply=0) and torch.equal(e.view(torch.int32), before_e.view(torch.int32))
        else:
            ds.append(got["d"])
    assert ref["updates"] == 40 and len(ds) == 40 and all(a <= b for a, b in zip(ds, ds[1:]))
    assert (ds[-1] == f32(decay) and ds[0] < f32(decay)) == switch_inside


# ---------------------------------------------------------------------------------------------------------------- models
def new_keypoint_net():
    from mdcv.rektnet.keypoint_net import KeypointNet
    zs = np.load(os.path.join(G, "rektnet_net.npz"))
    model = KeypointNet(7, (80, 80))
    model.load_state_dict({k[4:]: torch.from_numpy(zs[k]) for k in zs.files if k.startswith("sd::")})
    return model.cuda().train()


def new_darknet(precision="bf16"):
    from mdcv.yolo.models import Darknet
    cwd = os.getcwd()
    os.chdir(MINI)
    try:
        net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision=precision)
        net.load_weights("mini.weights", net.get_start_weight_dim())
    finally:
        os.chdir(cwd)
    return net.cuda().train()


def live_image(net, ema):
    """the live parameters and BatchNorm statistics in the shadow's layout (NumPy; a device read)"""
    out = np.zeros(ema._total, np.float32)
    out[:ema._n] = net.flat_parameters()[0].cpu().numpy()
    for (_, off, ln), t in zip(ema._rows, ema._stat_tensors(net)):
        out[off:off + ln] = t.detach().reshape(-1).cpu().numpy()
    return out


def mini_batches():
    z = np.load(os.path.join(G, "mini_darknet.npz"))
    x, tg = torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["targets"]).cuda()
    g = torch.Generator().manual_seed(6)
    return [x] + [torch.rand(x.shape, generator=g).cuda() for _ in range(5)], tg


@functools.lru_cache(maxsize=None)
def darknet_run(pipeline, with_ema=True, guarded=False, poison_at=None, leave_out=None):
    """6 steps of FusedAdam on the mini Darknet (a batch may be poisoned -- every gradient NaN -- or left out altogether).  With an EMA the
    shadow is compared with the restatement after EVERY step.  -> dict(live=[flat parameters after each step], shadow=..., block=..., ...)"""
    xs, tg = mini_batches()
    net = new_darknet()
    ema = WeightEMA(net, decay=0.5, warmup=3) if with_ema else None     # update 0 on the ramp (d = 1/3), the decay from update 1 on
    guard = GradGuard(skip_nonfinite=True) if guarded else None
    opt = FusedAdam(net, lr=1e-3, pipeline=pipeline, guard=guard, **({"ema": ema} if with_ema else {}))
    ref = R.new_block()
    E = live_image(net, ema) if with_ema else None
    if with_ema:
        assert same_bits(ema.shadow, E) and ema.updates == 0            # a copy of the live values, padding 0
    live, piped = [], False
    for i in range(6):
        if i == leave_out:
            continue
        opt.zero_grad()
        loss = net(xs[i], tg)[0].sum()
        if i == poison_at:
            loss = loss * float("nan")                                  # finite activations, every gradient NaN
        loss.backward()
        opt.step()
        piped = piped or getattr(net, "_pipe_plan", None) is not None
        live.append(net.flat_parameters()[0].clone())
        if with_ema:
            R.advance(ref, 0.5, 3, guard_apply=(0 if i == poison_at else 1) if guarded else None)
            R.update(ref, E, live_image(net, ema))
            assert same_bits(ema.shadow, E), (pipeline, i)
            assert block_equal(ema.block(), ref) == [], (pipeline, i)
    out = dict(live=live, piped=piped, net=net, opt=opt, ema=ema)
    if with_ema:
        out.update(shadow=ema.shadow.clone(), block=ema.block(), n=ema._n)
    return out


@pytest.mark.parametrize("pipeline", [False, True], ids=["plain", "pipelined"])
def test_mini_darknet_shadow_follows_the_restatement_and_the_live_weights_do_not_notice(pipeline):
    with_ema, without = darknet_run(pipeline), darknet_run(pipeline, with_ema=False)      # (the per-step comparison runs inside)
    assert with_ema["piped"] == pipeline and without["piped"] == pipeline
    assert with_ema["block"]["updates"] == 6 and with_ema["ema"].updates == 6
    assert len(with_ema["live"]) == 6 and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(with_ema["live"], without["live"]))
    assert not torch.equal(with_ema["shadow"][:with_ema["n"]], with_ema["live"][-1])     # an average, not a copy


def test_pipelined_shadow_equals_the_plain_shadow():
    a, b = darknet_run(False), darknet_run(True)
    assert b["piped"] and not a["piped"]
    assert torch.equal(a["shadow"].view(torch.int32), b["shadow"].view(torch.int32)) and a["block"] == b["block"]


@pytest.mark.parametrize("pipeline", [False, True], ids=["plain", "pipelined"])
def test_a_dropped_step_never_reaches_the_average(pipeline):
    got = darknet_run(pipeline, guarded=True, poison_at=2)
    want = darknet_run(pipeline, guarded=True, leave_out=2)
    assert got["opt"].guard.stats()["skipped"] == 1 and want["opt"].guard.stats()["skipped"] == 0
    assert got["block"]["updates"] == want["block"]["updates"] == 5 and got["block"]["d"] == want["block"]["d"]
    n = got["n"]
    # the flat part as bits.  (The BatchNorm segments cannot match: the poisoned batch's FORWARD moved the live running statistics before the
    # guard saw anything -- GradGuard's documented limit -- and the run compares them with the restatement on its own live values, step by step.)
    assert torch.equal(got["shadow"][:n].view(torch.int32), want["shadow"][:n].view(torch.int32))
    assert bool(torch.isfinite(got["shadow"]).all())
    # the live step right behind the dropped one is the clean run's
    assert torch.equal(got["live"][1], got["live"][2]) and torch.equal(got["live"][3], want["live"][2])


# ---------------------------------------------------------------------------------------------------------------- applied()
def three_steps(pipeline, decay=0.9):
    xs, tg = mini_batches()
    net = new_darknet()
    ema = WeightEMA(net, decay=decay, warmup=3)
    opt = FusedAdam(net, lr=1e-3, pipeline=pipeline, ema=ema)
    for i in range(3):
        opt.zero_grad()
        net(xs[i], tg)[0].sum().backward()
        opt.step()
    return net, ema, opt, xs, tg


def one_more_step(net, opt, xs, tg):
    opt.zero_grad()
    net(xs[3], tg)[0].sum().backward()
    opt.step()
    return net.flat_parameters()[0].clone()


@pytest.mark.parametrize("pipeline", [False, True], ids=["plain", "after_a_pipelined_step"])
def test_applied_swaps_the_averaged_model_in_and_back(pipeline):
    net, ema, opt, xs, tg = three_steps(pipeline)
    assert (getattr(net, "_pipe_plan", None) is not None) == pipeline
    averaged = {k: v.clone() for k, v in ema.averaged_state_dict().items()}
    assert len(averaged) == len(list(net.parameters())) + 2 * len(WeightEMA._bn_modules(net))
    other = new_darknet()
    other.load_state_dict({**other.state_dict(), **averaged})
    live_before = live_image(net, ema)
    shadow_before = ema.shadow.clone()
    with ema.applied():
        assert np.array_equal(u32(live_image(net, ema)), u32(shadow_before.cpu().numpy()))
        sd = net.state_dict()
        assert all(torch.equal(sd[k].view(torch.int32), v.view(torch.int32)) for k, v in averaged.items())
        net.eval(), other.eval()
        with torch.no_grad():
            got, want = net(xs[0]), other(xs[0])
        assert got.dtype == torch.float32 and torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))
        with pytest.raises(RuntimeError):
            ema.update()
        with pytest.raises(RuntimeError):
            opt.step()
        with pytest.raises(RuntimeError):
            with ema.applied():
                pass
        net.train()
    assert np.array_equal(u32(live_image(net, ema)), u32(live_before)) and torch.equal(ema.shadow.view(torch.int32), shadow_before.view(torch.int32))
    with torch.no_grad():                                               # ... and the averaged forward was not the live one
        net.eval()
        assert not torch.equal(net(xs[0]), got)
        net.train()
    # an exception inside still swaps back
    with pytest.raises(KeyError):
        with ema.applied():
            raise KeyError("inside")
    assert np.array_equal(u32(live_image(net, ema)), u32(live_before)) and torch.equal(ema.shadow.view(torch.int32), shadow_before.view(torch.int32))
    # training goes on as in the run that never entered it
    twin_net, twin_ema, twin_opt, _, _ = three_steps(pipeline)
    a, b = one_more_step(net, opt, xs, tg), one_more_step(twin_net, twin_opt, xs, tg)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(ema.shadow.view(torch.int32), twin_ema.shadow.view(torch.int32)) and ema.updates == twin_ema.updates == 4


def test_copy_to_and_reset():
    net, ema, opt, xs, tg = three_steps(False)
    shadow = ema.shadow.clone()
    ema.copy_to()
    assert np.array_equal(u32(live_image(net, ema)), u32(shadow.cpu().numpy())) and torch.equal(ema.shadow, shadow)
    one_more_step(net, opt, xs, tg)
    ema.reset()
    assert ema.updates == 0 and np.array_equal(u32(live_image(net, ema)), u32(ema.shadow.cpu().numpy()))


def keypoint_step(net, opt, seed):
    from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss
    with contextlib.redirect_stdout(io.StringIO()):
        crit = CrossRatioLoss("l1_softargmax", False, 0.05, 0.05)
    g = torch.Generator().manual_seed(seed)
    x, tp = torch.rand(4, 3, 80, 80, generator=g).cuda(), (torch.rand(4, 7, 2, generator=g) * 0.9).cuda()
    opt.zero_grad()
    out = net(x)
    crit(out[0], out[1], None, tp)[2].backward()
    opt.step()


@pytest.mark.parametrize("which", ["FusedSGD", "torch.optim.SGD"])
def test_sgd_and_a_torch_optimizer_update_the_average_and_it_follows_a_reflatten(which):
    from mdcv.optim import FusedSGD
    net = new_keypoint_net()
    ema = WeightEMA(net, decay=0.75, warmup=2)
    fused = which == "FusedSGD"
    opt = FusedSGD(net, lr=1e-2, momentum=0.9, ema=ema) if fused else torch.optim.SGD(net.parameters(), lr=1e-2, momentum=0.9)
    ref, E = R.new_block(), live_image(net, ema)

    def step_and_check(seed):
        keypoint_step(net, opt, seed)
        if not fused:
            ema.update()                                                # behind a torch optimizer the caller updates the average
        R.advance(ref, 0.75, 2)
        R.update(ref, E, live_image(net, ema))
        assert same_bits(ema.shadow, E) and block_equal(ema.block(), ref) == [], seed
    step_and_check(1)
    step_and_check(2)
    # re-pointed parameters and statistics: the model re-flattens, the table is rebuilt, the average goes on
    old_flat, old_table = net.flat_parameters()[0].data_ptr(), ema._table.clone()
    first = next(net.parameters())
    first.data = first.data.clone()
    net.bn.running_mean = net.bn.running_mean.clone()
    step_and_check(3)
    assert net.flat_parameters()[0].data_ptr() != old_flat and not torch.equal(ema._table, old_table) and ema.updates == 3
    # another layout is refused, both sizes named
    ema._n -= 4
    with pytest.raises(ValueError, match=r"%d.*%d" % (ema._n, ema._n + 4)):
        ema.update()
    ema._n += 4


# ---------------------------------------------------------------------------------------------------------------- state
def test_state_dict_round_trip_continues_with_identical_bits():
    net, ema, opt, xs, tg = three_steps(False)
    sd, msd = opt.state_dict(), {k: v.clone() for k, v in net.state_dict().items()}
    assert sd["ema"]["updates"] == 3 and sd["ema"]["decay"] == 0.9 and sd["ema"]["warmup"] == 3
    assert "ema" not in FusedAdam(new_keypoint_net(), lr=1e-3).state_dict()
    net2 = new_darknet()
    net2.load_state_dict(msd)
    ema2 = WeightEMA(net2, decay=0.5, warmup=7)
    opt2 = FusedAdam(net2, lr=1e-3, ema=ema2)
    opt2.load_state_dict(sd)
    assert (ema2.decay, ema2.warmup, ema2.updates) == (0.9, 3, 3) and torch.equal(ema2.shadow.view(torch.int32), ema.shadow.view(torch.int32))
    a, b = one_more_step(net, opt, xs, tg), one_more_step(net2, opt2, xs, tg)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(ema.shadow.view(torch.int32), ema2.shadow.view(torch.int32)) and ema.block() == ema2.block()
    # a shadow of another size
    kp = WeightEMA(new_keypoint_net())
    with pytest.raises(ValueError, match=r"%d.*%d" % (sd["ema"]["shadow"].numel(), kp.shadow.numel())):
        kp.load_state_dict(sd["ema"])
    assert kp.updates == 0


# ---------------------------------------------------------------------------------------------------------------- loops
def run_yolo_train(tmp_path, monkeypatch, name, **kw):
    from mdcv.yolo import train as yt
    root = tmp_path / name
    os.makedirs(root / "dataset")
    for f in ("mini.cfg", "mini.weights"):
        shutil.copy(os.path.join(MINI, f), root / f)
    anchors = open(os.path.join(MINI, "dataset", "train.csv")).readline()
    rows = open(os.path.join(G, "imgload", "dataset.csv")).read().splitlines()[1:]
    for f in ("train.csv", "validate.csv"):
        with open(root / "dataset" / f, "w") as fh:
            fh.write(anchors.rstrip("\n") + "\n" + "\n".join(rows) + "\n")
    z = np.load(os.path.join(G, "imgload", "frames.npz"))
    frames = {k: z[k] for k in z.files}
    monkeypatch.chdir(root)
    os.makedirs("out")
    args = dict(evaluate=False, batch_size=2, optimizer_pick="Adam", model_cfg="mini.cfg", weights_path="mini.weights", output_path="out",
                dataset_path="", num_epochs=2, num_steps=1000, checkpoint_interval=1, augment_affine=False, augment_hsv=False, lr_flip=False,
                ud_flip=False, momentum=0.9, gamma=0.95, lr=1e-3, weight_decay=0.0, vis_batch=0, data_aug=False, blur=False, salt=False,
                noise=False, contrast=False, sharpen=False, ts=False, debug_mode=False, upload_dataset=False, xy_loss=2.0, wh_loss=1.6,
                no_object_loss=25.0, object_loss=0.1, vanilla_anchor=False, val_tolerance=3, min_epochs=0, num_workers=1)
    lines, state, snaps = [], {}, {}

    def log(line):
        lines.append(line)
        if "weight EMA" in line:                                        # logged behind the live save, in front of the swap
            ema = state["optimizer"].ema
            snaps[state["epoch"]] = (live_image(state["model"], ema), ema.shadow.cpu().numpy().copy())
    with contextlib.redirect_stdout(io.StringIO()):
        yt.train(**args, decode=lambda p: frames[os.path.splitext(os.path.basename(p))[0]], log=log, state=state, **kw)
    return lines, state, snaps, root


def loaded_image(path):
    """a fresh mini Darknet that loaded `path`, in the shadow's layout"""
    net = new_darknet()
    net.load_weights(str(path), net.get_start_weight_dim())
    return live_image(net, WeightEMA(net))


def test_yolo_train_checkpoints_the_averaged_model_and_keeps_the_live_one(tmp_path, monkeypatch):
    lines, state, snaps, root = run_yolo_train(tmp_path, monkeypatch, "on", ema_decay=0.9, ema_warmup=3)
    ema = state["optimizer"].ema
    assert isinstance(ema, WeightEMA) and (ema.decay, ema.warmup) == (0.9, 3) and ema.updates == state["step"][0] > 0
    assert sorted(os.listdir(root / "out")) == ["1.live.weights", "1.weights", "2.live.weights", "2.weights"]
    extra = [l for l in lines if "weight EMA" in l]
    assert len(extra) == 2 and extra[0].startswith("train Epoch: 1, weight EMA: ") and f"{snaps_updates(extra[0])} updates" in extra[0]
    assert sorted(snaps) == [1, 2]
    for epoch in (1, 2):
        live, averaged = snaps[epoch]
        got_avg, got_live = loaded_image(root / "out" / f"{epoch}.weights"), loaded_image(root / "out" / f"{epoch}.live.weights")
        assert np.array_equal(u32(got_avg), u32(averaged)) and np.array_equal(u32(got_live), u32(live))
        assert not np.array_equal(u32(got_avg), u32(got_live))
    # the model is the live one again, and it was the averaged one that was validated
    assert np.array_equal(u32(live_image(state["model"], ema)), u32(snaps[2][0]))
    # off: the parent's files and lines
    off_lines, off_state, off_snaps, off_root = run_yolo_train(tmp_path, monkeypatch, "off")
    assert off_state["optimizer"].ema is None and off_snaps == {}
    assert sorted(os.listdir(off_root / "out")) == ["1.weights", "2.weights"] and not any("EMA" in l for l in off_lines)
    plain = [l for l in lines if "weight EMA" not in l]
    assert len(plain) == len(off_lines)

    def strip(l):                                                       # (the validation epochs see other weights: their numbers and verdicts differ)
        return l.split(", Total:")[0] if ", Total:" in l else "Validation loss" if l.startswith("Validation loss") else l.split(":")[0]
    assert [strip(l) for l in plain] == [strip(l) for l in off_lines]


def snaps_updates(line):
    return int(line.split("weight EMA: ")[1].split(" updates")[0])


def test_train_model_validates_the_averaged_keypoint_net_and_checkpoints_both(tmp_path, monkeypatch):
    from mdcv.data import SyntheticConeCrops
    from mdcv.rektnet import train as rt
    from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss
    from mdcv.rektnet.evaluate import eval_model
    with contextlib.redirect_stdout(io.StringIO()):
        crit = CrossRatioLoss("l1_softargmax", False, 0.05, 0.05)
    seen = []

    def recording_eval(**kw):
        out = eval_model(**kw)
        seen.append(out)
        return out
    monkeypatch.setattr(rt, "eval_model", recording_eval)
    train_data, val_data = SyntheticConeCrops(4, batches=3, seed=2), SyntheticConeCrops(4, batches=2, seed=3)
    net = new_keypoint_net()
    opt = FusedAdam(net, lr=1e-2)
    with contextlib.redirect_stdout(io.StringIO()):
        rt.train_model(net, str(tmp_path), train_data, crit, opt, torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.9), 2, val_data, 1, (80, 80), 7,
                       True, ["k"] * 7, "s", False, log=lambda l: None, ema_decay=0.5, ema_warmup=1)
        ema = opt.ema
        assert isinstance(ema, WeightEMA) and (ema.decay, ema.warmup, ema.updates) == (0.5, 1, 6) and len(seen) == 2
        with ema.applied():
            averaged_loss = eval_model(model=net, dataloader=val_data, loss_function=crit, input_size=(80, 80))
        live_loss = eval_model(model=net, dataloader=val_data, loss_function=crit, input_size=(80, 80))
    assert seen[-1] == averaged_loss and live_loss != averaged_loss
    files = [f for f in os.listdir(tmp_path) if f.endswith(".pt")]
    assert len(files) == 1 and files[0].startswith("1_loss_")
    ck = torch.load(os.path.join(tmp_path, files[0]), weights_only=False)
    assert ck["ema"]["updates"] == 6 and torch.equal(ck["ema"]["shadow"].cpu(), ema.shadow.cpu()) and "ema" in ck["optimizer"]
    live = net.state_dict()
    assert all(torch.equal(ck["model"][k].cpu(), v.cpu()) for k, v in live.items())                 # 'model' stays the live one
    # an optimizer that cannot take an EMA
    with pytest.raises(TypeError):
        rt.train_model(net, str(tmp_path), train_data, crit, torch.optim.Adam(net.parameters()), None, 1, val_data, 5, (80, 80), 7, False, [], "s",
                       False, ema_decay=0.9)
