"""-m gpu: a training plan audited launch by launch from its own tensors (tests/helpers/plan_audit.py has the reference and the bounds).

After one forward + backward every activation and every activation gradient of the step is still in the plan's buffers (a plan owns what it
touches, `plan.outs` / `plan.recs` keep the nodes), so every unit of the lowering is re-evaluated in float64 from the device's own tensors one
step upstream and compared element by element against derived bounds: a wiring mistake of engine.py / netplan.py / yolo/lower.py is an O(1) miss
of one unit, not noise under a tolerant end-to-end bar.  The counters of the plan prove which rewritten forms the audited run took; mutated launch
lists prove that a wrong plan fails, at its unit alone; the four backward schedules must leave identical bits.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import plan_audit as pa  # noqa: E402
import plan_audit_kpt as pk  # noqa: E402
from test_gpu_models import write_baseline_cfg  # noqa: E402
from test_plan_audit_host import make_case  # noqa: E402

D = torch.float64
SWITCHES = ("pw_fuse", "pw_fwd_px", "pw_bwd1", "fuse_bn", "fuse_skip", "stats_xacc", "first_conv_2pass")
FORCED_ON = dict(pw_fuse=True, pw_fwd_px=(0, 1 << 30), pw_bwd1=True, fuse_bn=True, fuse_skip=0, stats_xacc=True, first_conv_2pass=True)
FORCED_OFF = dict(pw_fuse=False, pw_fwd_px=(0, 1 << 30), pw_bwd1=False, fuse_bn=False, fuse_skip=0, stats_xacc=False, first_conv_2pass=False)
CONFIGS = {"default": ("bf16", {}), "forced_on": ("bf16", FORCED_ON), "forced_off": ("bf16", FORCED_OFF), "fp32": ("fp32", {})}


class switches:
    """class attributes of engine.Plan for the plans built inside the block"""

    def __init__(self, values):
        self.values = values

    def __enter__(self):
        from mdcv import engine
        self.saved = {k: getattr(engine.Plan, k) for k in SWITCHES}
        for k, v in self.values.items():
            setattr(engine.Plan, k, v)

    def __exit__(self, *exc):
        from mdcv import engine
        for k, v in self.saved.items():
            setattr(engine.Plan, k, v)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    out = {}
    for name in ("compact", "tiny"):
        tmp = tmp_path_factory.mktemp("audit_" + name)
        out[name] = (str(tmp),) + make_case(name, tmp)
    return out


def build_net(tmp, orc, params, precision):
    from mdcv.yolo.models import Darknet
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        cfg = [f for f in os.listdir(tmp) if f.endswith(".cfg")][0]
        net = Darknet(os.path.join(tmp, cfg), 2.0, 1.6, 25.0, 0.1, True, precision=precision)
    finally:
        os.chdir(cwd)
    with torch.no_grad():
        for i, L in enumerate(orc.layers):
            if L["type"] != "convolutional":
                continue
            m = net.module_list[i]
            m[0].weight.copy_(params[f"conv{i}.weight"].float())
            if L["bn"]:
                for leaf in ("weight", "bias", "running_mean", "running_var"):
                    getattr(m[1], leaf).copy_(params[f"bn{i}.{leaf}"].float())
            else:
                m[0].bias.copy_(params[f"conv{i}.bias"].float())
    return net.cuda()


def master_params(net, orc):
    """the masters as the device holds them (float32), as float64; running statistics included"""
    p = {}
    for i, L in enumerate(orc.layers):
        if L["type"] != "convolutional":
            continue
        m = net.module_list[i]
        p[f"conv{i}.weight"] = m[0].weight.detach().double().cpu()
        if L["bn"]:
            for leaf in ("weight", "bias", "running_mean", "running_var"):
                p[f"bn{i}.{leaf}"] = getattr(m[1], leaf).detach().double().cpu()
        else:
            p[f"conv{i}.bias"] = m[0].bias.detach().double().cpu()
    return p


def nchw(act, c):
    return act.dense()[..., :c].permute(0, 3, 1, 2).double().cpu().contiguous()


def bind(plan, graph, train):
    """plan.recs against the units of the cfg analysis, one to one and of the same kind (the lowering's own decisions -- which shortcut is folded --
    must be the ones the analysis predicts)"""
    units = [u for u in graph.units if train or u.kind != "YoloHead"]
    assert [type(r).__name__ for r in plan.recs] == [u.kind for u in units]
    for u, r in zip(units, plan.recs):
        if u.kind == "ConvBn":
            assert (r.resid is not None) == u.info["resid"], u
    return list(zip(units, plan.recs))


def read_plan(net, plan, graph, orc, train=True):
    torch.cuda.synchronize()
    t = pa.Tensors()
    pairs = bind(plan, graph, train)
    t.act["in"] = nchw(pairs[0][1].x.act, graph.chan["in"])
    for u, r in pairs:
        if u.out is None:
            continue
        node = plan.outs[u.out]
        t.act[u.out] = nchw(node.act, graph.chan[u.out])
        if train and node.grad is not None:
            t.grad[u.out] = nchw(node.grad, graph.chan[u.out])
        if u.kind == "ConvBn" and train:
            t.y[u.sec] = nchw(r.y, u.info["cout"])
            t.mean[u.sec], t.invstd[u.sec] = r.bs.mean.double().cpu(), r.bs.invstd.double().cpu()
    if train:
        for i, L in enumerate(orc.layers):
            if L["type"] != "convolutional":
                continue
            m = net.module_list[i]
            t.pgrad[f"conv{i}.weight"] = m[0].weight.grad.double().cpu()
            if L["bn"]:
                t.pgrad[f"bn{i}.weight"], t.pgrad[f"bn{i}.bias"] = m[1].weight.grad.double().cpu(), m[1].bias.grad.double().cpu()
            else:
                t.pgrad[f"conv{i}.bias"] = m[0].bias.grad.double().cpu()
        t.out7 = plan.out7.double().cpu()
    return t


def train_step(net, x, tg):
    net.train()
    net.zero_grad(set_to_none=True)
    out = net(x.cuda(), tg.cuda())
    out[0].backward()
    torch.cuda.synchronize()
    return [p for p in net._plans.values() if p.has_bwd][0]


def counters(plan):
    return dict(fused_bn=int(plan.fused_bn), pw_fwd_count=int(getattr(plan, "pw_fwd_count", 0)), pw_bwd1_count=int(getattr(plan, "pw_bwd1_count", 0)),
                stats_xfolded=int(plan.stats_xfolded), first_conv_fwd2=int(bool(getattr(plan, "first_conv_fwd2", False))),
                deferred_reduces=sum(r == 3 for r in plan._classify_bwd()))


def audit(P, graph, params, tens, tg, orc, what, **kw):
    rep = pa.Report()
    pa.audit_darknet(P, graph, params, tens, tg, pa.hyper_of(orc), rep, **kw)
    print(f"plan audit error / bound on the device ({what}):", {f"{k[0]}.{k[1]}": round(v, 4) for k, v in sorted(rep.worst_by_kind().items())})
    return rep


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", ["compact", "tiny"])
def test_training_plan_unit_by_unit(cases, name, config):
    tmp, orc, graph, params, x, tg = cases[name]
    precision, sw = CONFIGS[config]
    with switches(sw):
        net = build_net(tmp, orc, params, precision)
        plan = train_step(net, x, tg)
    cnt = counters(plan)
    print(f"plan audit counters ({name}, {config}):", cnt)
    if config == "forced_off" or precision == "fp32":
        off = ("pw_fwd_count", "pw_bwd1_count", "first_conv_fwd2", "deferred_reduces", "fused_bn") + (("stats_xfolded",) if config == "forced_off" else ())
        assert all(cnt[k] == 0 for k in off), cnt
    elif name == "compact":
        must = tuple(cnt) if config == "forced_on" else ("fused_bn", "stats_xfolded", "first_conv_fwd2", "pw_bwd1_count", "deferred_reduces")
        assert all(cnt[k] > 0 for k in must), cnt
    else:                                                    # (the tiny cfg's widths admit no 1x1 form and its first conv is not the 32-filter one)
        assert cnt["stats_xfolded"] > 0 and cnt["fused_bn"] > 0, cnt
    P = pa.Prec(precision == "bf16")
    tens = read_plan(net, plan, graph, orc)
    assert torch.equal(tens.act["in"], P.store(x.float()).double())
    rep = audit(P, graph, master_params(net, orc), tens, tg, orc, f"{name}, {config}")
    rep.assert_clean(f"{name} / {config}")
    assert len(rep.rows) > 5 * len(graph.units) // 2


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["compact", "tiny"])
def test_eval_plan_unit_by_unit(cases, name, precision):
    """inference plans: conv + BatchNorm(running statistics) + activation in one launch, decoded rows; the running statistics are not the initial ones"""
    tmp, orc, graph, params, x, tg = cases[name]
    net = build_net(tmp, orc, params, precision).eval()
    with torch.no_grad():
        rows = net(x.cuda())
    plan = [p for p in net._plans.values() if not p.has_bwd][0]
    names = [getattr(f, "__name__", "") for f, _ in plan.fwd]
    assert sum("conv2d_affine_act" in n for n in names) == sum(u.kind == "ConvBn" for u in graph.units), names
    assert sum("yolo_head_decode" in n for n in names) == sum(u.kind == "YoloHead" for u in graph.units)
    P = pa.Prec(precision == "bf16")
    tens = read_plan(net, plan, graph, orc, train=False)
    tens.rows = rows.double().cpu()
    rep = audit(P, graph, master_params(net, orc), tens, None, orc, f"{name}, eval {precision}", train=False, bn_eval=True)
    rep.assert_clean(f"{name} / eval {precision}")
    assert any(r[1] == "rows" for r in rep.rows)


# ------------------------------------------------------------------------------------------------ a wrong plan must fail, at its unit
def _entry(lst, fns, *ptrs):
    hits = [k for k, (f, a) in enumerate(lst) if any(f is g for g in fns) and all(p in a for p in ptrs)]
    assert len(hits) == 1, hits
    return hits[0]


def _swap(lst, k, old, new):
    f, a = lst[k]
    assert a.count(old) == 1
    lst[k] = (f, tuple(new if v == old else v for v in a))


def test_mutated_launch_lists_fail_at_their_unit_only(cases):
    tmp, orc, graph, params, x, tg = cases["compact"]
    net = build_net(tmp, orc, params, "bf16")
    xs = [x, torch.rand(x.shape, generator=torch.Generator().manual_seed(11))]      # alternate: what a dropped launch leaves behind is the OTHER input's
    plan = train_step(net, xs[0], tg)
    L, P = plan.L, pa.Prec(True)
    recs = {u.sec: r for u, r in bind(plan, graph, True)}
    applies = (L.bn_act_fwd, L.bn_act_fwd_xstats)
    masters = master_params(net, orc)
    step = [0]

    def run(expect):
        step[0] += 1
        xx = xs[step[0] % 2]
        assert train_step(net, xx, tg) is plan
        rep = audit(P, graph, masters, read_plan(net, plan, graph, orc), tg, orc, f"mutation, expected at {sorted(expect)}")
        charged = rep.missed_sections()
        assert charged, f"the mutation at {sorted(expect)} passed the audit"
        assert all(s & expect for s in charged) and any(s <= expect for s in charged), (sorted(expect), [sorted(s) for s in charged], rep.format_misses())

    def restored():
        """one step of the restored lists between two edits (the backward runner caches the stream roles of a list by its length)"""
        step[0] += 1
        assert train_step(net, xs[step[0] % 2], tg) is plan

    # (a) the residual of the apply of sections 10 + 11 (node 8) -> node 5: same shape, same ldc, live
    r = recs[10]
    old, new = r.resid.act, plan.outs[5].act
    assert (old.B, old.H, old.W, old.C, old.ldc) == (new.B, new.H, new.W, new.C, new.ldc) and old.ptr != new.ptr and new.off == 0
    assert new.buf.numel() >= new.M * new.ldc
    k = _entry(plan.fwd, applies, r.y.ptr, old.ptr)
    keep = plan.fwd[k]
    _swap(plan.fwd, k, old.ptr, new.ptr)
    run({10})
    plan.fwd[k] = keep
    restored()
    # (b) one finalize of the fused BatchNorm-backward sums dropped (reads and writes less than before)
    fins = [k for k, (f, a) in enumerate(plan.bwd) if f is L.bn_bwd_finalize_rows]
    assert fins
    k = fins[len(fins) // 2]
    sec = [s for s, r in recs.items() if type(r).__name__ == "ConvBn" and r.bs.cA.data_ptr() in plan.bwd[k][1]]
    assert len(sec) == 1
    keep = plan.bwd.pop(k)
    run({sec[0]})
    plan.bwd.insert(k, keep)
    restored()
    # (c) the add that joins the two consumers (shortcut 19, route 31) of conv 18's gradient dropped
    g18 = plan.outs[18].grad
    adds = [k for k, (f, a) in enumerate(plan.bwd) if f is L.bn_act_fwd and a[3] is None and a[11] == g18.ptr]
    assert len(adds) == 1, adds
    keep = plan.bwd.pop(adds[0])
    run({19, 31})
    plan.bwd.insert(adds[0], keep)
    restored()
    # (d) conv 18 writes its slice of route 31's concat buffer 8 channels low: still inside the buffer's rows
    r = recs[18]
    z = r.z.act
    assert z is plan.outs[18].act and z.off >= 8 and z.off - 8 + z.C <= z.ldc and z.buf.numel() >= z.M * z.ldc
    k = _entry(plan.fwd, applies, r.y.ptr, z.ptr)
    keep = plan.fwd[k]
    _swap(plan.fwd, k, z.ptr, z.ptr - 8 * z.buf.element_size())
    run({18})
    plan.fwd[k] = keep
    # and the restored plan is clean again
    step[0] += 1
    train_step(net, xs[step[0] % 2], tg)
    audit(P, graph, masters, read_plan(net, plan, graph, orc), tg, orc, "restored").assert_clean("restored plan")


# ------------------------------------------------------------------------------------------------ schedules
SCHEDULES = [("serial", dict(overlap_wgrad=False)), ("overlapped", {}), ("no fork on dispatch", dict(fork_on_dispatch=False)),
             ("no deferred reduces", dict(defer_slab_reduce=False))]


def _schedules_identical(net, x, tg):
    from mdcv import netplan
    NP = netplan._NetPlan
    saved = {k: getattr(NP, k) for k in ("overlap_wgrad", "fork_on_dispatch", "defer_slab_reduce")}
    got = {}
    try:
        for rnd in range(2):
            for name, sw in SCHEDULES:
                for k, v in {**dict(overlap_wgrad=True, fork_on_dispatch=True, defer_slab_reduce=True), **sw}.items():
                    setattr(NP, k, v)
                plan = train_step(net, x, tg)
                got.setdefault(name, []).append((net.flat_parameters()[1].clone(), plan.out7.clone(), sum(r == 3 for r in plan._classify_bwd())))
    finally:
        for k, v in saved.items():
            setattr(NP, k, v)
    ref_g, ref_o, _ = got["serial"][0]
    assert float(ref_g.abs().max()) > 0 and bool(torch.isfinite(ref_g).all())
    for name, runs in got.items():
        for g, o, _ in runs:
            assert torch.equal(o, ref_o), name
            assert torch.equal(g, ref_g), (name, int((g != ref_g).sum()))
    assert got["overlapped"][0][2] > 0 and got["no deferred reduces"][0][2] == 0        # the switch reached the classifier
    return got


def test_schedules_leave_identical_bits_compact(cases):
    tmp, orc, graph, params, x, tg = cases["compact"]
    _schedules_identical(build_net(tmp, orc, params, "bf16"), x, tg)


def test_schedules_leave_identical_bits_yolo_baseline(tmp_path):
    from mdcv.yolo.models import Darknet
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        torch.manual_seed(3)
        net = Darknet(write_baseline_cfg(str(tmp_path), 416, 80), 2.0, 1.6, 25.0, 0.1, True, precision="bf16").cuda()
    finally:
        os.chdir(cwd)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 416, 416, generator=g)
    tg = torch.zeros(2, 4, 5)
    tg[:, :2, 1:3] = torch.rand(2, 2, 2, generator=g) * 0.9 + 0.05
    tg[:, :2, 3:5] = torch.rand(2, 2, 2, generator=g) * 0.28 + 0.02
    _schedules_identical(net, x, tg)


# ------------------------------------------------------------------------------------------------ KeypointNet
def build_keypoint(sd, precision):
    from mdcv.rektnet.keypoint_net import KeypointNet
    kp = KeypointNet(7, (80, 80), precision=precision)
    kp.load_state_dict({**kp.state_dict(), **{k: v.float() for k, v in sd.items()}})
    return kp.cuda()


def read_keypoint(kp, plan, train):
    from mdcv import engine
    torch.cuda.synchronize()
    sd = {k: v.detach().double().cpu() for k, v in kp.state_dict().items() if "num_batches" not in k}
    co = lambda cv: sd[f"{cv}.weight"].shape[0]       # noqa: E731
    T = pk.KTensors()
    recs = plan.recs
    assert [r[0] for r in recs] == ["stem"] + ["block"] * 4
    _, cs0, bs0, xin, y0, a0 = recs[0]
    T.act["in"], T.act["a0"] = nchw(xin.act, 3), nchw(a0.act, co("conv"))
    ys, bss, nodes = {"conv": y0}, {"bn": bs0}, {"a0": a0}
    for r, rec in enumerate(recs[1:], start=1):
        _, x, cs1, bs1, y1, mid, cs2, bs2, y2, css, bss_, ysc, out = rec
        assert x is nodes[f"a{r - 1}"]                                        # (the block reads the node the record before it wrote)
        nodes[f"m{r}"], nodes[f"a{r}"] = mid, out
        T.act[f"m{r}"], T.act[f"a{r}"] = nchw(mid.act, co(f"res{r}.conv1")), nchw(out.act, co(f"res{r}.conv2"))
        ys.update({f"res{r}.conv1": y1, f"res{r}.conv2": y2, f"res{r}.shortcut_conv": ysc})
        bss.update({f"res{r}.bn1": bs1, f"res{r}.bn2": bs2, f"res{r}.shortcut_bn": bss_})
    T.y = {k: nchw(v, co(k)) for k, v in ys.items() if v is not None}
    L = plan.L
    sm = [a for f, a in plan.fwd if f is L.softargmax_fwd]
    assert len(sm) == 1
    ptr, ldc = sm[0][1], sm[0][2]
    buf = [t for t in list(plan.keep) + [getattr(plan, "lg32", None)] if isinstance(t, torch.Tensor) and t.data_ptr() == ptr]
    assert buf
    T.lg = buf[0].reshape(-1)[:4 * 80 * 80 * ldc].view(4, 80, 80, ldc)[..., :7].permute(0, 3, 1, 2).double().cpu().contiguous()
    T.hm, T.pts = plan.hm.double().cpu(), plan.pts.double().cpu()
    if train:
        T.mean = {k: v.mean.double().cpu() for k, v in bss.items()}
        T.invstd = {k: v.invstd.double().cpu() for k, v in bss.items()}
        T.grad = {k: nchw(v.grad, T.act[k].shape[1]) for k, v in nodes.items()}
        T.pgrad = {k: p.grad.double().cpu() for k, p in kp.named_parameters()}
        T.dpts = plan.dpts.double().cpu()
        dlg = [c.cell_contents for c in plan.bwd[0][0].__closure__ if isinstance(c.cell_contents, engine.Act)]
        assert len(dlg) == 1
        T.dlg = nchw(dlg[0], 7)
    return sd, T


def _kpt_report(P, sd, T, what, train=True):
    rep = pa.Report()
    pk.audit_keypoint(P, sd, T, rep, train=train)
    w = {f"{k[0]}.{k[1]}": v for k, v in rep.worst_by_kind().items()}
    print(f"plan audit error / bound on the device (KeypointNet, {what}):", {k: round(v, 4) for k, v in sorted(w.items())})
    return rep


@pytest.mark.parametrize("config", list(CONFIGS))
def test_keypoint_training_plan_unit_by_unit(config):
    from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss
    precision, sw = CONFIGS[config]
    sd0 = pk.keypoint_state(3)
    x, tpts = pk.keypoint_batch()
    with switches(sw):
        kp = build_keypoint(sd0, precision).train()
        hm, pts = kp(x.cuda())
        CrossRatioLoss("l1_softargmax", True, 0.05, 0.05)(hm, pts, None, tpts.cuda())[2].backward()
    plan = [p for p in kp._plans.values() if p.has_bwd][0]
    cnt = counters(plan)
    print(f"plan audit counters (KeypointNet, {config}):", cnt)
    if config == "forced_off" or precision == "fp32":
        assert all(cnt[k] == 0 for k in ("pw_fwd_count", "pw_bwd1_count", "first_conv_fwd2", "deferred_reduces", "fused_bn")), cnt
    else:
        # production default and forced on: the 3x3 data gradients carry BatchNorm sums, a 1x1 shortcut conv takes the one-launch backward and
        # its slab reduce is deferred.  The other three forms cannot fire on this net:
        assert cnt["fused_bn"] > 0 and cnt["pw_bwd1_count"] > 0 and cnt["deferred_reduces"] > 0, cnt
        assert cnt["pw_fwd_count"] == 0, cnt        # its 1x1 convs read block outputs written by the dual-BatchNorm apply, which no conv can absorb
        assert cnt["stats_xfolded"] == 0, cnt       # the KeypointNet builder allocates no accumulator arena
        assert cnt["first_conv_fwd2"] == 0, cnt     # the stem is 7x7 with 16 filters; the two-pass kernel is 3x3 with 32
    P = pa.Prec(precision == "bf16")
    sd, T = read_keypoint(kp, plan, True)
    assert torch.equal(T.act["in"], P.store(x.float()).double())
    rep = _kpt_report(P, sd, T, config)
    rep.assert_clean(f"KeypointNet / {config}")
    assert len(rep.rows) > 100


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_keypoint_inference_plan_unit_by_unit(precision):
    sd0 = pk.keypoint_state(3)
    x, _ = pk.keypoint_batch()
    kp = build_keypoint(sd0, precision).eval()
    with torch.no_grad():
        kp(x.cuda())
    plan = [p for p in kp._plans.values() if not p.has_bwd][0]
    names = [getattr(f, "__name__", "") for f, _ in plan.fwd]
    assert sum("conv2d_affine_act" in n for n in names) == 5, names           # stem + conv1 of every block
    sd, T = read_keypoint(kp, plan, False)
    rep = _kpt_report(pa.Prec(precision == "bf16"), sd, T, f"inference {precision}", train=False)
    rep.assert_clean(f"KeypointNet / inference {precision}")
    assert len(rep.rows) >= 20
