"""-m gpu: the gradient guard (csrc/grad_guard.hip, mdcv.optim.GradGuard) against its NumPy restatement (tests/gradguard_ref.py), as bits:
the fp64 sum of squares and the control block, the skip of a non-finite step, the guarded Adam / SGD updates over a sequence with a poisoned
step in it, clipping, the guarded against the unguarded update inside the fp64 error bound, the "as if the batch never happened" property
on KeypointNet and a pipelined mini Darknet, and the training loop's one extra line."""
import contextlib
import io
import math
import os
import shutil

import numpy as np
import pytest
import torch

import gradguard_ref as R

pytestmark = pytest.mark.gpu

from mdcv import _lib  # noqa: E402
from mdcv.optim import FusedAdam, FusedSGD, GradGuard, grad_norm  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MINI = os.path.join(G, "mini")
f32 = np.float32
U = 2.0 ** -24
BLOCK_FIELDS = ("sumsq", "norm", "coef", "scale", "bc1", "bc2_sqrt", "finite", "apply", "attempted", "applied", "skipped", "clipped", "max_norm")


def st():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(t, a):
    """device fp32 tensor == NumPy fp32 array, bit for bit (signed zeros and denormals included)"""
    got, want = t.detach().cpu().numpy(), np.asarray(a, np.float32)
    nan = np.isnan(want)                 # (a NaN a host operation CREATES carries the host's sign bit: NaNs are compared as NaNs)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def block_equal(got, want):
    bad = []
    for k in BLOCK_FIELDS:
        g, w = float(got[k]), float(want[k])
        if not (g == w or (math.isnan(g) and math.isnan(w))):
            bad.append((k, g, w))
    return bad


def wide(n, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros(n, np.float32)
    g = np.clip(rng.standard_normal(n) * 10.0 ** rng.uniform(-44, 38, n), -3e38, 3e38).astype(np.float32)      # denormals .. 3e38
    fixed = np.array([1e-45, -3e38, 3e38, -1e-45, 1.1754942e-38], np.float32)
    pos = rng.permutation(n)[:fixed.size]
    g[pos] = fixed[:pos.size]
    return g


# ---------------------------------------------------------------------------------------------------------------- sumsq and finalize
SIZES = [1, 3, 255, 256, 257, 4095, 4096, 4097, R.MAX_GRID * R.CHUNK + 5]      # the last: the workgroups stride over the chunks


@pytest.mark.parametrize("n,kind", [(n, "wide") for n in SIZES] + [(3, "zero"), (4097, "zero")], ids=str)
def test_sumsq_and_finalize_equal_the_restatement(n, kind):
    g = wide(n, n, kind)
    gd = torch.from_numpy(g).cuda()
    gs, max_norm, betas = 1.0 / 32, 1.0, (0.9, 0.999)
    guard = GradGuard(max_norm=max_norm, ring=4)
    guard.measure(gd, gs, betas)
    parts = guard._partials[:(n + R.CHUNK - 1) // R.CHUNK].cpu().numpy()
    want_parts = R.sumsq_partials(g)
    assert np.array_equal(parts.view(np.uint64), want_parts.view(np.uint64))
    got = guard.stats()
    want = R.finalize(R.new_block(), g, gs, max_norm, True, *betas, ring=4)
    assert block_equal(got, want) == []
    assert got["norms"] == [float(want["norm"])] and float(guard.norm) == float(want["norm"])
    assert got["finite"] == 1 and got["apply"] == 1
    # another launch context: a side stream, the raw entry points, scratch of its own -- the same bits
    L = _lib.lib()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        p2 = torch.full((parts.size + 3,), -1.0, dtype=torch.float64, device="cuda")
        blk = torch.zeros(9, dtype=torch.int64, device="cuda")
        L.check(L.grad_sumsq(gd.data_ptr(), n, p2.data_ptr(), side.cuda_stream))
        L.check(L.grad_guard_finalize(p2.data_ptr(), parts.size, gs, max_norm, 1, float(f32(0.9)), float(f32(0.999)), blk.data_ptr(), None, 0,
                                      side.cuda_stream))
    side.synchronize()
    assert torch.equal(p2[:parts.size].cpu(), guard._partials[:parts.size].cpu()) and bool((p2[parts.size:] == -1.0).all())
    assert torch.equal(blk.cpu(), guard._buf[:9].cpu())
    # grad_scale's sign does not enter the norm; scale keeps it
    guard.measure(gd, -gs, betas)
    again = guard.stats()
    assert again["norm"] == got["norm"] and again["scale"] == -got["scale"] and again["attempted"] == 2


def test_bad_arguments_are_refused_before_any_launch():
    L = _lib.lib()
    g = torch.zeros(64, device="cuda")
    p = torch.zeros(4, dtype=torch.float64, device="cuda")
    blk = torch.zeros(9, dtype=torch.int64, device="cuda")
    assert L.grad_sumsq(g.data_ptr() + 4, 8, p.data_ptr(), st()) == -1 and L.grad_sumsq(g.data_ptr(), 0, p.data_ptr(), st()) == -1
    assert L.grad_sumsq(None, 8, p.data_ptr(), st()) == -1 and L.grad_sumsq(g.data_ptr(), 8, None, st()) == -1
    assert L.grad_guard_finalize(p.data_ptr(), 0, 1.0, 0.0, 1, 0.9, 0.999, blk.data_ptr(), None, 0, st()) == -1
    assert L.grad_guard_finalize(p.data_ptr(), 1, 1.0, 0.0, 1, 1.0, 0.999, blk.data_ptr(), None, 0, st()) == -1
    assert L.grad_guard_finalize(p.data_ptr(), 1, 1.0, 0.0, 1, 0.9, 0.999, blk.data_ptr(), None, 4, st()) == -1
    t = [torch.zeros(16, device="cuda") for _ in range(4)]
    assert L.adam_step_guarded(*[x.data_ptr() for x in t], 8, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, st()) == -1
    assert L.adam_step_guarded(t[0].data_ptr() + 4, *[x.data_ptr() for x in t[1:]], 8, blk.data_ptr(), 1e-3, 0.9, 0.999, 1e-8, 0.0, st()) == -1
    assert L.sgd_step_guarded(t[0].data_ptr(), t[1].data_ptr(), None, 8, blk.data_ptr(), 1e-2, 0.9, 0.0, st()) == -1
    torch.cuda.synchronize()
    assert int(blk.abs().sum()) == 0


# ---------------------------------------------------------------------------------------------------------------- raw optimizer state
class AdamState:
    """p, g, m, v on the device and in NumPy, one guard, one restated block"""

    def __init__(self, n, seed, guard, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0, gs=1.0):
        rng = np.random.default_rng(seed)
        self.n, self.rng, self.guard, self.gs = n, rng, guard, gs
        self.hyp = (lr, betas[0], betas[1], eps, wd)
        self.P = rng.standard_normal(n).astype(np.float32)
        self.M, self.V = np.zeros(n, np.float32), np.zeros(n, np.float32)
        self.p, self.m, self.v = (torch.from_numpy(a.copy()).cuda() for a in (self.P, self.M, self.V))
        self.g = torch.zeros(n, device="cuda")
        self.blk = R.new_block()

    def gradient(self, poison=None):
        G_ = (self.rng.standard_normal(self.n) / self.gs).astype(np.float32)
        if poison is not None:
            G_[poison[0]] = poison[1]
        return G_

    def step(self, G_):
        L = _lib.lib()
        self.g.copy_(torch.from_numpy(G_))
        self.guard.measure(self.g, self.gs, self.hyp[1:3])
        L.check(L.adam_step_guarded(self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n, self.guard.block_ptr,
                                    *self.hyp, st()))
        R.finalize(self.blk, G_, self.gs, self.guard.max_norm, self.guard.skip_nonfinite, self.hyp[1], self.hyp[2], ring=self.guard.ring)
        R.adam_step(self.blk, self.P, G_, self.M, self.V, *self.hyp)

    def check(self):
        assert block_equal(self.guard.stats(), self.blk) == []
        assert same_bits(self.p, self.P) and same_bits(self.m, self.M) and same_bits(self.v, self.V)


# ---------------------------------------------------------------------------------------------------------------- non-finite gradients
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("pos", [0, 4095, 4096], ids=["first", "last_vector_element", "scalar_tail"])
def test_a_non_finite_gradient_is_seen_and_the_step_skipped(pos, bad):
    s = AdamState(4097, 3, GradGuard(skip_nonfinite=True))
    s.step(s.gradient())
    s.check()
    before = [bits(t).clone() for t in (s.p, s.m, s.v)]
    c0 = s.guard.stats()
    s.step(s.gradient(poison=(pos, bad)))
    c1 = s.guard.stats()
    assert c1["finite"] == 0 and c1["apply"] == 0 and not math.isfinite(c1["sumsq"]) and not math.isfinite(c1["norm"])
    assert c1["applied"] == c0["applied"] == 1 and c1["skipped"] == c0["skipped"] + 1 == 1 and c1["attempted"] == 2
    assert all(torch.equal(bits(t), b) for t, b in zip((s.p, s.m, s.v), before))         # byte-identical
    s.check()
    # without skip_nonfinite the update runs: today's behaviour, the parameters show it
    k = AdamState(4097, 3, GradGuard(skip_nonfinite=False))
    k.step(k.gradient())
    k.step(k.gradient(poison=(pos, bad)))
    c = k.guard.stats()
    assert c["finite"] == 0 and c["apply"] == 1 and c["applied"] == 2 and c["skipped"] == 0
    assert bool(torch.isnan(k.p[pos])) and bool(torch.isnan(k.m[pos]) | torch.isinf(k.m[pos]))
    k.check()


# ---------------------------------------------------------------------------------------------------------------- guarded Adam and SGD
N_OPT = 1029          # two workgroups of the Adam grid, 257 float4 and a scalar tail of one


@pytest.mark.parametrize("gs", [1.0, 1.0 / 32], ids=["gs1", "gs1/32"])
@pytest.mark.parametrize("wd", [0.0, 5e-4], ids=["wd0", "wd5e-4"])
def test_guarded_adam_sequence_equals_the_restatement(wd, gs):
    s = AdamState(N_OPT, 7, GradGuard(skip_nonfinite=True, ring=8), wd=wd, gs=gs)
    s.step(s.gradient()); s.check()                                                    # noqa: E702
    s.step(s.gradient()); s.check()                                                    # noqa: E702
    s.step(s.gradient(poison=(5, float("nan")))); s.check()                            # noqa: E702
    assert s.blk["applied"] == 2 and s.blk["skipped"] == 1
    s.step(s.gradient()); s.check()                                                    # noqa: E702
    want = R.bias_corrections(np.float64(f32(0.9)), np.float64(f32(0.999)), 3)          # t = applied + 1 = 3, not the 4th attempt
    got = s.guard.stats()
    assert (got["bc1"], got["bc2_sqrt"]) == (float(want[0]), float(want[1])) and got["applied"] == 3
    # a late state: 999 steps applied (what a resumed run loads), the moments as they stand
    late = dict(attempted=1000, applied=999, skipped=1, clipped=0, max_norm=float(s.blk["max_norm"]))
    s.guard.load_state_dict(late)
    s.blk.update(late, max_norm=f32(late["max_norm"]))
    s.step(s.gradient()); s.check()                                                    # noqa: E702
    assert s.guard.stats()["applied"] == 1000 and len(s.guard.stats()["norms"]) == 8


class SgdState(AdamState):
    def __init__(self, n, seed, guard, lr=1e-2, momentum=0.9, wd=0.0, gs=1.0):
        super().__init__(n, seed, guard, wd=wd, gs=gs)
        self.hyp = (lr, momentum, wd)
        self.M[:] = 7.0                                                                # a stale buffer: the first applied step must not read it
        self.m.fill_(7.0)

    def step(self, G_):
        L = _lib.lib()
        self.g.copy_(torch.from_numpy(G_))
        self.guard.measure(self.g, self.gs)
        L.check(L.sgd_step_guarded(self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.n, self.guard.block_ptr, *self.hyp, st()))
        R.finalize(self.blk, G_, self.gs, self.guard.max_norm, self.guard.skip_nonfinite, ring=self.guard.ring)
        R.sgd_step(self.blk, self.P, G_, self.M, *self.hyp)


@pytest.mark.parametrize("gs", [1.0, 1.0 / 32], ids=["gs1", "gs1/32"])
@pytest.mark.parametrize("wd", [0.0, 5e-4], ids=["wd0", "wd5e-4"])
@pytest.mark.parametrize("mom", [0.0, 0.9], ids=["mom0", "mom0.9"])
def test_guarded_sgd_sequence_equals_the_restatement(mom, wd, gs):
    s = SgdState(N_OPT, 8, GradGuard(), momentum=mom, wd=wd, gs=gs)
    s.step(s.gradient(poison=(N_OPT - 1, float("inf")))); s.check()                    # noqa: E702   the FIRST attempt is skipped
    assert s.blk["applied"] == 0 and bool((s.m == 7.0).all())
    s.step(s.gradient()); s.check()                                                    # noqa: E702   first APPLIED step: buf = gradient
    if mom:
        assert not bool((s.m == 7.0).any())
    s.step(s.gradient()); s.check()                                                    # noqa: E702
    s.step(s.gradient(poison=(0, float("nan")))); s.check()                            # noqa: E702
    s.step(s.gradient()); s.check()                                                    # noqa: E702
    assert (s.blk["attempted"], s.blk["applied"], s.blk["skipped"]) == (5, 3, 2)
    assert bool(torch.isfinite(s.p).all())


# ---------------------------------------------------------------------------------------------------------------- clipping
def test_clipping_scales_the_step_and_counts_only_clipped_steps():
    s = AdamState(N_OPT, 9, GradGuard(max_norm=4.0))
    G_ = s.gradient()                                                                  # norm ~ sqrt(1029) ~ 32 > 4
    s.step(G_); s.check()                                                              # noqa: E702
    c = s.guard.stats()
    assert c["norm"] > 4.0 and c["coef"] < 1.0 and c["clipped"] == 1 and c["scale"] == c["coef"]
    assert abs(c["coef"] * c["norm"] - 4.0) <= 4 * U * 4.0
    small = (G_ * f32(1.0 / 64)).astype(np.float32)                                    # norm ~ 0.5 < 4: the coefficient is exactly 1
    s.step(small); s.check()                                                           # noqa: E702
    c = s.guard.stats()
    assert c["norm"] < 4.0 and c["coef"] == 1.0 and c["scale"] == 1.0 and c["clipped"] == 1 and c["applied"] == 2
    assert c["max_norm"] == s.guard.stats()["norms"][0]
    s.step(s.gradient(poison=(3, float("inf")))); s.check()                            # noqa: E702   a skipped step is not a clipped one
    assert s.guard.stats()["clipped"] == 1


# ---------------------------------------------------------------------------------------------------------------- guarded vs unguarded
def w64(t):
    return t.detach().double().cpu()


def _bc_err(beta, step):
    """relative error of a bias correction 1 - beta^t formed in fp32 on the host: powf within 1 ulp (2 u beta^t), the subtraction (u)"""
    bt = beta ** step
    return 0.0 if step == 1 else 2 * U * bt / (1 - bt) + U


@pytest.mark.parametrize("gs,wd", [(1.0, 0.0), (1.0 / 32, 5e-4)], ids=str)
def test_untriggered_guard_and_unguarded_update_agree_within_the_fp64_bound(gs, wd):
    """The guarded kernel rounds every operation on its own, the unguarded one lets the compiler contract: they may differ in the last
    bit.  Both must lie inside the error bound of the fp64 update -- k roundings of relative size u against the terms' absolute values,
    as counted below -- and hence within twice that bound of each other."""
    L = _lib.lib()
    n = N_OPT
    rng = np.random.default_rng(21)
    lr, b1, b2, eps, wdf, gsf = (float(f32(x)) for x in (1e-3, 0.9, 0.999, 1e-8, wd, gs))
    p0_ = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
    runs = {}
    for which in ("plain", "guarded"):
        runs[which] = dict(p=p0_.clone(), m=torch.zeros(n, device="cuda"), v=torch.zeros(n, device="cuda"))
    guard = GradGuard(max_norm=1e30, skip_nonfinite=True)                              # attached, never triggered: coef == 1
    grng = np.random.default_rng(22)
    for step in (1, 2, 3, 1000):            # three consecutive steps, then a late one; every step starts both runs from the SAME state
        for key in ("p", "m", "v"):
            runs["guarded"][key].copy_(runs["plain"][key])
        if step == 1000:
            guard.load_state_dict(dict(attempted=999, applied=999))
        gr = torch.from_numpy((grng.standard_normal(n) / gs).astype(np.float32)).cuda()
        Gd = w64(gr)
        after = {}
        for which, s in runs.items():
            p0, m0, v0 = w64(s["p"]), w64(s["m"]), w64(s["v"])
            if which == "guarded":
                guard.measure(gr, gsf, (b1, b2))
                L.check(L.adam_step_guarded(s["p"].data_ptr(), gr.data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), n, guard.block_ptr,
                                            lr, b1, b2, eps, wdf, st()))
            else:
                L.check(L.adam_step(s["p"].data_ptr(), gr.data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), n, step, lr, b1, b2, eps, wdf, gsf, st()))
            torch.cuda.synchronize()
            grad = Gd * gsf + wdf * p0
            ga = (Gd * gsf).abs() + (wdf * p0).abs()
            mr, ma = b1 * m0 + (1 - b1) * grad, (b1 * m0).abs() + (1 - b1) * ga
            vr, va = b2 * v0 + (1 - b2) * grad * grad, b2 * v0 + (1 - b2) * ga * ga
            bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
            den = torch.sqrt(vr) / math.sqrt(bc2) + eps
            pr = p0 - (lr / bc1) * mr / den
            # m: 7 roundings (the gradient: 3; 1 - beta1, two products, the sum); v: 10 (the gradient twice); the update: m's 7, half of v's
            # 10 under the root, 6 for lr / bc1, the root, the quotients, the product and the sum, plus the bias corrections' own error
            bm, bv = 7 * U * ma, 10 * U * va
            ua = (lr / bc1) * ma / den
            rel = (7 + 5 + 6) * U + _bc_err(b1, step) + 0.5 * _bc_err(b2, step) + 0.5 * 10 * U * (va / vr.clamp_min(1e-300) - 1)
            bp = U * torch.maximum(p0.abs(), pr.abs()) + rel * ua
            em, ev, ep = (w64(s["m"]) - mr).abs() / bm.clamp_min(1e-300), (w64(s["v"]) - vr).abs() / bv.clamp_min(1e-300), \
                (w64(s["p"]) - pr).abs() / bp.clamp_min(1e-300)
            assert float(em.max()) <= 1.0 and float(ev.max()) <= 1.0 and float(ep.max()) <= 1.0, (which, step, float(em.max()), float(ev.max()), float(ep.max()))
            after[which] = (bm, bv, bp)
        c = guard.stats()
        assert c["coef"] == 1.0 and c["scale"] == gsf and c["clipped"] == 0 and c["skipped"] == 0 and c["applied"] == step
        # same start, same fp64 reference, each inside the bound about it: within twice the bound of each other
        for key, k in (("m", 0), ("v", 1), ("p", 2)):
            d = (w64(runs["guarded"][key]) - w64(runs["plain"][key])).abs()
            lim = after["guarded"][k] + after["plain"][k]
            assert float((d / lim.clamp_min(1e-300)).max()) <= 1.0, (key, step)


# ---------------------------------------------------------------------------------------------------------------- models
def new_keypoint_net():
    from mdcv.rektnet.keypoint_net import KeypointNet
    zs = np.load(os.path.join(G, "rektnet_net.npz"))
    model = KeypointNet(7, (80, 80))
    model.load_state_dict({k[4:]: torch.from_numpy(zs[k]) for k in zs.files if k.startswith("sd::")})
    return model.cuda().train()


def new_darknet(precision=None):
    from mdcv.yolo.models import Darknet
    cwd = os.getcwd()
    os.chdir(MINI)
    try:
        net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, **({} if precision is None else {"precision": precision}))
        net.load_weights("mini.weights", net.get_start_weight_dim())
    finally:
        os.chdir(cwd)
    return net.cuda().train()


def keypoint_run(bad_at, pipeline):
    """steps over batches 0, 1, 2 (bad_at: the index of a batch whose heat-map target is all NaN for one sample, or None: that batch is
    left out altogether) -> (flat parameters after each APPLIED step, the guard's stats)"""
    from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss
    with contextlib.redirect_stdout(io.StringIO()):
        crit = CrossRatioLoss("l2_heatmap", False, 0.05, 0.05)
    g = torch.Generator().manual_seed(4)
    xs = [torch.rand(4, 3, 80, 80, generator=g).cuda() for _ in range(3)]
    hms = [torch.rand(4, 7, 80, 80, generator=g).cuda() for _ in range(3)]
    tp = (torch.rand(4, 7, 2, generator=g) * 0.9).cuda()
    net = new_keypoint_net()
    opt = FusedAdam(net, lr=1e-3, pipeline=pipeline, guard=GradGuard())
    snaps = []
    for i in range(3):
        hm_t = hms[i]
        if i == 1:
            if bad_at is None:
                continue
            hm_t = hm_t.clone()
            hm_t[2] = float("nan")
        opt.zero_grad()
        out = net(xs[i])
        crit(out[0], out[1], hm_t, tp)[2].backward()
        opt.step()
        if i != 1:
            snaps.append(net.flat_parameters()[0].clone())
    return snaps, opt.guard.stats(), net


@pytest.mark.parametrize("pipeline", [False, True], ids=["plain", "pipelined"])
def test_keypointnet_survives_a_nan_heatmap_as_if_the_batch_never_happened(pipeline):
    got, stats, net = keypoint_run(1, pipeline)
    want, clean, _ = keypoint_run(None, pipeline)
    assert stats["skipped"] == 1 and stats["applied"] == 2 and stats["attempted"] == 3 and clean["skipped"] == 0 and clean["applied"] == 2
    assert bool(torch.isfinite(net.flat_parameters()[0]).all())
    assert len(got) == len(want) == 2 and all(torch.equal(a, b) for a, b in zip(got, want))
    assert not torch.equal(got[0], got[1])
    assert math.isnan(stats["norms"][1]) and all(math.isfinite(stats["norms"][k]) for k in (0, 2))
    gn = grad_norm(net)                                                                # the last batch's gradient is still in place
    assert float(gn) == stats["norm"] and gn.is_cuda and gn.dtype == torch.float32


def darknet_run(bad_at, pipeline=True):
    z = np.load(os.path.join(G, "mini_darknet.npz"))
    x, tg = torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["targets"]).cuda()
    g = torch.Generator().manual_seed(6)
    xs = [x] + [torch.rand(x.shape, generator=g).cuda() for _ in range(2)]
    net = new_darknet("bf16")
    opt = FusedAdam(net, lr=1e-3, pipeline=pipeline, guard=GradGuard())
    snaps = []
    for i in range(3):
        if i == 1 and bad_at is None:
            continue
        opt.zero_grad()
        loss = net(xs[i], tg)[0].sum()
        if i == 1:
            loss = loss * float("nan")                                                 # finite activations, every gradient NaN
        loss.backward()
        opt.step()
        if i != 1:
            snaps.append(net.flat_parameters()[0].clone())
    return snaps, opt.guard.stats(), net, opt


def test_pipelined_darknet_survives_a_nan_gradient_as_if_the_batch_never_happened():
    got, stats, net, opt = darknet_run(1)
    want, clean, _, _ = darknet_run(None)
    assert getattr(net, "_pipe_plan", None) is not None                                 # the update did run in pipelined groups
    assert stats["skipped"] == 1 and stats["applied"] == 2 and clean["skipped"] == 0
    assert bool(torch.isfinite(net.flat_parameters()[0]).all())
    assert len(got) == 2 and all(torch.equal(a, b) for a, b in zip(got, want))
    # a checkpoint carries the counters, and a resumed optimizer bias-corrects with the applied count
    sd = opt.state_dict()
    assert sd["step"] == 3 and sd["guard"] == dict(attempted=3, applied=2, skipped=1, clipped=0, max_norm=stats["max_norm"])
    net2 = new_darknet("bf16")
    opt2 = FusedAdam(net2, lr=1e-3, guard=GradGuard())
    opt2.load_state_dict(sd)
    assert opt2.guard.stats()["applied"] == 2
    opt2.step()
    c = opt2.guard.stats()
    want_bc = R.bias_corrections(np.float64(f32(0.9)), np.float64(f32(0.999)), 3)
    assert (c["applied"], c["attempted"], c["bc1"], c["bc2_sqrt"]) == (3, 4, float(want_bc[0]), float(want_bc[1]))
    assert "guard" not in FusedAdam(net2, lr=1e-3).state_dict()


# ---------------------------------------------------------------------------------------------------------------- loop and CLI
def yolo_batches(n, B=2, T=4, seed=5):
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(n):
        x = torch.rand(B, 3, 64, 64, generator=g)
        t = torch.zeros(B, T, 5)
        for b in range(B):
            m = 1 + (k + b) % T
            t[b, :m, 1:3] = 0.1 + 0.8 * torch.rand(m, 2, generator=g)
            t[b, :m, 3:5] = 0.05 + 0.3 * torch.rand(m, 2, generator=g)
        out.append(([f"img{k}_{b}" for b in range(B)], x.cuda(), t.cuda()))
    return out


def test_run_epoch_logs_one_summary_line_and_still_waits_once():
    from mdcv.yolo.train import run_epoch
    runs = {}
    for name, guard in (("none", None), ("guard", GradGuard(max_norm=1e30, skip_nonfinite=True))):
        net = new_darknet()
        lines, stats = [], {}
        ret = run_epoch("train", yolo_batches(5), 100, FusedAdam(net, lr=1e-3, guard=guard), net, 3, 9, [0], log=lines.append, stats=stats)
        runs[name] = (lines, stats, ret)
    plain, guarded = runs["none"][0], runs["guard"][0]
    assert len(plain) == 6 and not any("grad norm" in l for l in plain)
    assert len(guarded) == 7 and guarded[-1].startswith("train Epoch: 3, grad norm max ")
    assert guarded[-1].endswith(", clipped 0, skipped 0 of 5 steps") and " mean " in guarded[-1]
    # the reference's lines: the first step's is the same string (same parameters, same batch); all of them keep their form
    assert guarded[:2] == plain[:2]
    assert all(l.startswith(f"train Epoch: 3, Batch: {k}/5, Total:") for k, l in enumerate(guarded[1:6], 1))
    assert runs["none"][1] == {"host_waits": 1, "steps": 5} and runs["guard"][1] == {"host_waits": 1, "steps": 5}
    # a second epoch reports its own steps
    net = new_darknet()
    opt = FusedAdam(net, lr=1e-3, guard=GradGuard(max_norm=1e-3))
    for epoch in (1, 2):
        lines = []
        run_epoch("train", yolo_batches(3), 100, opt, net, epoch, 2, [0], log=lines.append)
        assert lines[-1].startswith(f"train Epoch: {epoch}, grad norm max ") and lines[-1].endswith(", clipped 3, skipped 0 of 3 steps")
    assert opt.guard.stats()["clipped"] == 6


def test_train_model_logs_the_summary_line_and_takes_the_keywords(tmp_path):
    from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss
    from mdcv.rektnet.train import train_model
    with contextlib.redirect_stdout(io.StringIO()):
        crit = CrossRatioLoss("l1_softargmax", False, 0.05, 0.05)
    g = torch.Generator().manual_seed(9)
    batches = [(torch.rand(4, 3, 80, 80, generator=g).cuda(), torch.zeros(4, 7, 80, 80, device="cuda"), (torch.rand(4, 7, 2, generator=g) * 0.9).cuda(),
                ["c"] * 4, [(80, 80, 3)] * 4) for _ in range(2)]
    outs = {}
    for name, kw in (("none", {}), ("guard", dict(clip_grad_norm=1e-4, skip_nonfinite=True))):
        net = new_keypoint_net()
        opt = FusedAdam(net, lr=1e-3)
        lines, stats = [], {}
        with contextlib.redirect_stdout(io.StringIO()):
            train_model(net, str(tmp_path), batches, crit, opt, torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.9), 1, batches[:1], 5, (80, 80), 7,
                        False, ["k"] * 7, "s", False, log=lines.append, stats=stats, **kw)
        outs[name] = (lines, stats, opt)
    assert not any("grad norm" in l for l in outs["none"][0]) and outs["none"][2].guard is None
    lines, stats, opt = outs["guard"]
    assert [l for l in lines if "grad norm" in l] == [l for l in lines if l.endswith(", clipped 2, skipped 0 of 2 steps")] and stats["host_waits"] == [1]
    assert lines.index([l for l in lines if "grad norm" in l][0]) == 2 and lines[1].startswith("\tTraining:")
    assert opt.guard.max_norm == 1e-4 and opt.guard.skip_nonfinite is True
    with pytest.raises(TypeError):
        train_model(net, str(tmp_path), batches, crit, torch.optim.Adam(net.parameters()), None, 1, batches[:1], 5, (80, 80), 7, False, [], "s", False,
                    clip_grad_norm=1.0)


def test_command_line_flags_reach_the_optimizer(tmp_path, monkeypatch):
    from mdcv.yolo import train as yt
    opt = yt._parser().parse_args(["--model_cfg", "mini.cfg"])
    assert opt.clip_grad_norm == 0.0 and opt.skip_nonfinite is False
    seen = {}
    monkeypatch.setattr(yt, "train", lambda **kw: seen.update(kw))
    yt.main(["--model_cfg", "mini.cfg", "--clip_grad_norm", "10", "--skip_nonfinite"])
    assert seen["clip_grad_norm"] == 10.0 and seen["skip_nonfinite"] is True
    yt.main(["--model_cfg", "mini.cfg", "--no_skip_nonfinite"])
    assert seen["clip_grad_norm"] == 0.0 and seen["skip_nonfinite"] is False
    monkeypatch.undo()
    # ... and train() hands them to the optimizer it builds
    for name in ("mini.cfg", "mini.weights"):
        shutil.copy(os.path.join(MINI, name), tmp_path / name)
    os.makedirs(tmp_path / "dataset")
    anchors = open(os.path.join(MINI, "dataset", "train.csv")).readline()
    rows = open(os.path.join(G, "imgload", "dataset.csv")).read().splitlines()[1:]
    for name in ("train.csv", "validate.csv"):
        with open(tmp_path / "dataset" / name, "w") as f:
            f.write(anchors.rstrip("\n") + "\n" + "\n".join(rows) + "\n")
    z = np.load(os.path.join(G, "imgload", "frames.npz"))
    frames = {k: z[k] for k in z.files}
    monkeypatch.chdir(tmp_path)
    os.makedirs("out")
    args = dict(evaluate=False, batch_size=2, optimizer_pick="SGD", model_cfg="mini.cfg", weights_path="mini.weights", output_path="out",
                dataset_path="", num_epochs=1, num_steps=1000, checkpoint_interval=1, augment_affine=False, augment_hsv=False, lr_flip=False,
                ud_flip=False, momentum=0.9, gamma=0.95, lr=1e-3, weight_decay=0.0, vis_batch=0, data_aug=False, blur=False, salt=False,
                noise=False, contrast=False, sharpen=False, ts=False, debug_mode=False, upload_dataset=False, xy_loss=2.0, wh_loss=1.6,
                no_object_loss=25.0, object_loss=0.1, vanilla_anchor=False, val_tolerance=3, min_epochs=0, num_workers=1)
    lines, state = [], {}
    with contextlib.redirect_stdout(io.StringIO()):
        yt.train(**args, decode=lambda p: frames[os.path.splitext(os.path.basename(p))[0]], log=lines.append, state=state,
                 clip_grad_norm=10.0, skip_nonfinite=True)
    guard = state["optimizer"].guard
    assert isinstance(state["optimizer"], FusedSGD) and guard.max_norm == 10.0 and guard.skip_nonfinite is True
    assert guard.stats()["attempted"] == state["step"][0] == 2
    assert sum("grad norm" in l for l in lines) == 1                                   # the training epoch's; the validation epoch has no optimizer
