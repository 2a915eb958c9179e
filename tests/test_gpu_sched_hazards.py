"""-m gpu: the launch schedule of a training step is free of unordered buffer conflicts -- proved on the host from what a real step enqueued
(tests/helpers/sched_hazards.py has the recorder, the extent table and the analysis).

A recorder stands in for the library object before the model and its plans are built.  Two consecutive training steps (forward, backward,
optimizer step) are recorded -- a conflict between the next forward and a side-stream weight gradient, or between a parameter group and the
forward that reads its packed operands, only exists in a two-step window -- and every pair of launches that touch the same bytes, at least one
writing, must be ordered by the forks, arms, waits and events that were enqueued.  Nothing here depends on timing: no step is repeated to catch
a rare divergence, no wall-clock is read.

Networks: the compact cfg of the plan audit (128 x 160, B = 2), the tiny cfg of test_gpu_models.write_tiny_cfg with its own widths (16 .. 1024:
its 1024 -> 256 and 256 -> 128 1x1 layers take the one-launch backward) at 32 x 32, its smallest legal size (five stride-2 pools: the size is a
multiple of 32; at 32 the heads see 1 x 1 and 2 x 2 grids), B = 2, KeypointNet 80 x 80 (B = 3) and the production yolo_baseline wiring at 416^2
(B = 2): the forms the lowering picks depend on geometry.

Every (network, optimizer kind) pair is a model of its own, so no test inherits planted wait_params entries or a pipelined step in flight from
another kind, and a recording takes its wrappers off the plan's launch lists again when it ends.

Out of scope: data-parallel runs (the reducer's comm stream needs several processes), hipGraph mode (a captured list runs on one stream) and
the loaders' staging streams.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import plan_audit_kpt as pk  # noqa: E402
import sched_hazards as sh  # noqa: E402
from test_gpu_models import write_tiny_cfg  # noqa: E402
from test_gpu_plan_audit import SCHEDULES, build_keypoint, build_net  # noqa: E402
from test_plan_audit_host import make_case, tiny_targets  # noqa: E402

NETWORKS = ("compact", "tiny", "keypoint", "yolo_baseline")
SWITCHES_ON = dict(overlap_wgrad=True, fork_on_dispatch=True, defer_slab_reduce=True)


# ------------------------------------------------------------------------------------------------ recorder in place, networks under it
@pytest.fixture(scope="module")
def rec():
    from mdcv import _lib
    mp = pytest.MonkeyPatch()
    r = sh.Recorder(_lib.lib())
    mp.setattr(_lib, "_lib", r)            # launch lists bind L.<fn> objects at emit time: in place BEFORE any model of this module is built
    try:
        yield r
    finally:
        mp.undo()


class Net:
    """one network with its inputs and the step the driver runs on it"""

    def __init__(self, name, tmp):
        self.name = name
        if name == "compact":
            orc, _, params, x, tg = make_case(name, tmp)
            self.model = build_net(str(tmp), orc, params, "bf16").train()
            self.inputs = [x[:2].contiguous().cuda(), tg[:2].contiguous().cuda()]
        elif name == "tiny":
            from mdcv.yolo.models import Darknet
            cwd = os.getcwd()
            os.chdir(tmp)
            try:
                torch.manual_seed(1)
                self.model = Darknet(write_tiny_cfg(str(tmp), 32, 1), 2.0, 1.6, 25.0, 0.1, True, precision="bf16").cuda().train()
            finally:
                os.chdir(cwd)
            self.inputs = [torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(2)).cuda(), tiny_targets().cuda()]
        elif name == "yolo_baseline":
            sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
            import bench
            from mdcv.yolo.models import Darknet
            cwd = os.getcwd()
            os.chdir(tmp)
            try:
                torch.manual_seed(3)
                self.model = Darknet(bench.write_yolo_cfg(str(tmp), size=416), 2.0, 1.6, 25.0, 0.1, True, precision="bf16").cuda().train()
            finally:
                os.chdir(cwd)
            g = torch.Generator().manual_seed(5)
            tg = torch.zeros(2, 4, 5)
            tg[:, :2, 1:3] = torch.rand(2, 2, 2, generator=g) * 0.9 + 0.05
            tg[:, :2, 3:5] = torch.rand(2, 2, 2, generator=g) * 0.28 + 0.02
            self.inputs = [torch.rand(2, 3, 416, 416, generator=g).cuda(), tg.cuda()]
        else:
            self.model = build_keypoint(pk.keypoint_state(3), "bf16").train()
            g = torch.Generator().manual_seed(9)
            self.inputs = [torch.rand(3, 3, 80, 80, generator=g).cuda(), (torch.rand(3, 7, 2, generator=g) - 0.5).cuda()]

    def step(self, opt=None):
        opt = self.opt if opt is None else opt
        self.model.zero_grad(set_to_none=True)
        if self.name == "keypoint":
            _, pts = self.model(self.inputs[0])
            (pts * self.inputs[1]).sum().backward()
        else:
            self.model(*self.inputs)[0].backward()
        opt.step()

    @property
    def plan(self):
        return self.model._last_train_plan


@pytest.fixture(scope="module")
def nets(rec, tmp_path_factory):
    """(network, optimizer kind) -> a model of its own with its one optimizer (`net.opt`)"""
    from mdcv.optim import FusedAdam, GradGuard, WeightEMA
    cache = {}

    def get(name, kind="plain"):
        if (name, kind) not in cache:
            net = cache[name, kind] = Net(name, tmp_path_factory.mktemp("sched_" + name))
            kw = dict(guard=GradGuard(max_norm=1.0), ema=WeightEMA(net.model, decay=0.99, warmup=2)) if kind == "guard+ema" else {}
            net.opt = FusedAdam(net.model, lr=1e-4, pipeline=kind != "plain", **kw)
        return cache[name, kind]
    return get


class switches:
    def __init__(self, values):
        self.values = {**SWITCHES_ON, **values}

    def __enter__(self):
        from mdcv import netplan
        self.saved = {k: getattr(netplan._NetPlan, k) for k in self.values}
        for k, v in self.values.items():
            setattr(netplan._NetPlan, k, v)

    def __exit__(self, *exc):
        from mdcv import netplan
        for k, v in self.saved.items():
            setattr(netplan._NetPlan, k, v)


def record(rec, net, opt=None, steps=2):
    """one warm step (plans, streams, parameter groups), then `steps` recorded ones -> (trace, allocations, analysis)"""
    opt = net.opt if opt is None else opt
    net.step(opt)
    net.model._param_sync()                # every group of the warm step launched and joined: the recording starts from a quiet device
    torch.cuda.synchronize()
    rec.trace, rec.unmodelled, rec._keep = [], [], []
    with pytest.MonkeyPatch.context() as mp:
        rec.patch_torch(mp)
        rec.on = True
        try:
            for k in range(steps):
                rec.step = k + 1
                rec.wrap_lists(net.plan)   # (the first pipelined step plants wait_params entries: positions are taken anew per step)
                rec.hook_plan(net.plan)
                net.step(opt)
        finally:
            rec.on = False
            rec.unwrap(net.plan)
    net.model._param_sync()
    torch.cuda.synchronize()
    allocs = sh.Allocations()
    allocs.collect(net.model, "model")
    allocs.collect(opt, "optimizer")
    allocs.collect(net.inputs, "inputs")
    assert rec.unmodelled == [], f"launch-list entries that made no library call and have no row in TORCH_ENTRIES: {rec.unmodelled}"
    assert rec.resolve(allocs) == []
    trace = rec.trace
    return trace, allocs, sh.analyse(trace, allocs)


def launches(trace, **kw):
    return [r for r in trace if r["op"] == "launch" and all(r.get(k) == v for k, v in kw.items())]


def deferred_reduces(trace, step=1):
    """slab reduces of the one-launch 1x1 backward that were enqueued BEHIND a later entry of the backward list: they waited for a later fork"""
    n, top = 0, -1
    for r in launches(trace, step=step):
        e = r.get("entry")
        if e is None or e[0] != "bwd":
            continue
        if r["name"] == "wgrad_reduce" and e[1] < top:
            n += 1
        top = max(top, e[1])
    return n


def assert_clean(res, what):
    assert res.violations == [], (what, res.violations[:5])
    assert res.findings == [], (what, len(res.findings), res.findings[:8])


# ------------------------------------------------------------------------------------------------ a. the four backward schedules
@pytest.mark.parametrize("schedule", [s[0] for s in SCHEDULES])
@pytest.mark.parametrize("name", NETWORKS)
def test_backward_schedules_have_no_unordered_conflict(rec, nets, name, schedule):
    """Two steps with FusedAdam(pipeline=False) under each schedule of test_gpu_plan_audit.SCHEDULES: zero findings.  Not vacuous: the overlapped
    schedules put launches on the side stream and the analysis had cross-stream conflicts to order; the default schedule arms dispatches and
    defers exactly the slab reduces _classify_bwd gives role 3; the serial schedule is one stream (nothing to order is then the whole statement)."""
    net = nets(name)
    with switches(dict(SCHEDULES)[schedule]):
        trace, allocs, res = record(rec, net)
        roles = net.plan._classify_bwd()
    side = net.plan.side().cuda_stream if schedule != "serial" else None
    n_side = len(launches(trace, stream=side)) if side is not None else 0
    deferred = deferred_reduces(trace)
    print(f"sched-hazards {name} / {schedule}: {res.counts()} side-stream launches {n_side} deferred reduces (step 1) {deferred} "
          f"findings {len(res.findings)}")
    assert_clean(res, (name, schedule))
    assert res.launches > 20
    if schedule == "serial":
        assert res.streams == 1 and res.arms == 0 and n_side == 0
        return
    assert res.streams == 2 and n_side > 0 and res.cross_pairs > 0
    assert deferred == sum(r == 3 for r in roles)
    if schedule == "overlapped":
        assert res.arms > 0 and res.arms == 2 * sum(r == 1 for r in roles)
        assert deferred > 0                                  # every network has 1x1 layers that take the one-launch backward
    if schedule == "no fork on dispatch":
        assert res.arms == 0
    if schedule == "no deferred reduces":
        assert deferred == 0


# ------------------------------------------------------------------------------------------------ b. the pipelined optimizer
@pytest.mark.parametrize("extras", ["plain", "guard+ema"])
@pytest.mark.parametrize("name", ["compact", "yolo_baseline"])
def test_pipelined_optimizer_has_no_unordered_conflict(rec, nets, name, extras):
    """FusedAdam(pipeline=True), alone and with GradGuard + WeightEMA: parameter groups update and re-pack on a third stream, the late ones
    launched from the next forward's wait_params.  Zero findings over the two-step window: pflat ranges, wf / wd, the moments, the guard block,
    the EMA shadow and block (read by late groups of step N against the writes of step N + 1)."""
    net = nets(name, "pipelined" if extras == "plain" else extras)
    opt = net.opt
    with switches({}):
        trace, allocs, res = record(rec, net)
    pstream = opt._pstream.cuda_stream
    updates = [r for r in launches(trace, stream=pstream) if r["name"].startswith("adam_step")]
    late = [r for r in updates if r["entry"] is not None and r["entry"][2] == "wait_params"]
    print(f"sched-hazards {name} / pipelined {extras}: {res.counts()} parameter-stream launches {len(launches(trace, stream=pstream))} "
          f"group updates {len(updates)} of them from wait_params {len(late)} findings {len(res.findings)}")
    assert_clean(res, (name, extras))
    assert res.streams >= 3 and res.cross_pairs > 0
    # the window holds: step 1's two early groups, step 1's late groups (launched from step 2's forward), step 2's two early groups
    n = len(net.plan.param_groups)
    assert n >= 3 and len(updates) == n + 2 and len(late) == n - 2 and all(r["step"] == 2 for r in late)
    # the clean result rests on the events and on the wait_stream in front of the groups: without either (on the host) it is not clean
    main = torch.cuda.current_stream().cuda_stream
    no_waits = sh.analyse([dict(r) for r in trace if not (r["op"] == "wait" and r["stream"] == main)], allocs)
    assert [f for f in no_waits.findings if f.kind == "hazard" and f.earlier["stream"] == pstream and f.later["stream"] == main and
            f.earlier["name"] == "pack_weights_batched"], no_waits.findings[:4]
    no_join = sh.analyse([dict(r) for r in trace if not (r["op"] == "fork" and r["dst"] == pstream)], allocs)
    assert [f for f in no_join.findings if f.kind == "hazard" and f.later["name"].startswith("adam_step") and f.later["stream"] == pstream and
            f.label.startswith("RAW")], no_join.findings[:4]
    names = {r["name"] for r in trace if r["op"] == "launch"}
    if extras == "guard+ema":
        assert {"grad_sumsq", "grad_guard_finalize", "adam_step_guarded", "ema_advance", "ema_update", "ema_update_segments"} <= names
        assert all(r["name"] == "adam_step_guarded" for r in updates)
        assert len([r for r in launches(trace, stream=pstream) if r["name"] == "ema_update"]) == len(updates)
    else:
        assert "adam_step" in names and "pack_weights_batched" in names


# ------------------------------------------------------------------------------------------------ c. the recorder does not change the step
def test_recorder_does_not_change_the_step(rec, tmp_path_factory):
    """one seed, three steps: the flat gradient and parameters after a recorded run equal a run on the bare library, bit for bit"""
    from mdcv import _lib
    from mdcv.optim import FusedAdam
    got = []
    for recorded in (True, False):
        with pytest.MonkeyPatch.context() as mp:
            if not recorded:
                mp.setattr(_lib, "_lib", rec.real)
            net = Net("compact", tmp_path_factory.mktemp("sched_same"))
            assert isinstance(net.model._plans, dict) and (_lib.lib() is rec) == recorded
            opt = FusedAdam(net.model, lr=1e-3, pipeline=False)
            with switches({}):
                if recorded:
                    trace, _, res = record(rec, net, opt)
                    assert res.launches > 20 and net.plan.L is rec
                else:
                    for _ in range(3):
                        net.step(opt)
                    assert net.plan.L is rec.real
            p, g = net.model.flat_parameters()
            torch.cuda.synchronize()
            got.append((p.clone(), g.clone()))
    assert float(got[0][1].abs().max()) > 0 and bool(torch.isfinite(got[0][0]).all())
    assert torch.equal(got[0][1], got[1][1]), int((got[0][1] != got[1][1]).sum())
    assert torch.equal(got[0][0], got[1][0]), int((got[0][0] != got[1][0]).sum())


# ------------------------------------------------------------------------------------------------ d. one kernel per armed call
@pytest.mark.parametrize("name", NETWORKS)
def test_armed_calls_launch_exactly_one_kernel(rec, nets, name):
    """The armed event rides on the FIRST kernel of the next library call (csrc/common.h MDCV_LAUNCH): an entry _classify_bwd gives role 1 must
    launch exactly one kernel, or the side stream starts one kernel early.  Counted with the in-library profiler in a pass of its own.
    Limit: the profiler sees what goes through MDCV_LAUNCH.  A raw hipLaunchKernelGGL or a hipMemsetAsync inside an armed entry would not be
    counted (neither bn_bwd.hip nor pw_bwd.hip has one today; a memset would not take the armed event either, a raw kernel launch would not)."""
    from mdcv import engine
    net = nets(name)
    with switches({}):
        net.step()
        net.model._param_sync()
        torch.cuda.synchronize()
        plan = net.plan
        roles = plan._classify_bwd()
        timed = engine.run_timed(plan, plan.bwd, kernels=True)
    torch.cuda.synchronize()
    armed = [(i, t[0], len(t[3])) for i, (t, r) in enumerate(zip(timed, roles)) if r == 1]
    print(f"sched-hazards {name}: {len(armed)} armed entries of {len(roles)}, kernels per armed entry {sorted({n for _, _, n in armed})}")
    assert len(armed) > 0 and len(timed) == len(roles)
    assert [a for a in armed if a[2] != 1] == []


# ------------------------------------------------------------------------------------------------ e. declared write sets are true
@pytest.fixture(scope="module")
def compact_default(rec, nets):
    net = nets("compact")
    with switches({}):
        trace, allocs, res = record(rec, net)
    assert_clean(res, "compact default")
    return net, trace, allocs


def test_declared_write_sets_hold_every_changed_byte(rec, compact_default):
    """one recorded call per distinct (entry, form), replayed alone between two snapshots of every known allocation: each byte that changed
    lies inside the call's declared write set"""
    net, trace, allocs = compact_default
    order = sorted(allocs.by_base)
    views = [sh.byte_view(allocs.by_base[b][3]) for b in order]
    offs, total = {}, 0
    for b, v in zip(order, views):
        offs[b] = total
        total += v.numel()
    forms = {}
    for r in launches(trace):
        if not r.get("torch"):
            forms.setdefault(sh.form_of(r["name"], sh.named_args(rec.directions, r["name"], r["args"] + (None,))), r)
    assert len(forms) >= 20 and {"conv2d", "pw_bwd", "conv2d_wgrad", "wgrad_reduce", "bn_act_bwd_apply", "adam_step"} <= {f[0] for f in forms}
    st = torch.cuda.current_stream().cuda_stream
    bad = []
    for form, r in forms.items():
        declared = torch.zeros(total, dtype=torch.bool, device="cuda")
        written = torch.zeros(total, dtype=torch.bool, device="cuda")
        touched = set()
        for lab, p, nrows, pitch, used, mode in r["acc"]:
            al = allocs.resolve(p)
            touched.add(al[1])
            for m in (declared, written) if "w" in mode else (declared,):
                torch.as_strided(m, (nrows, used), (pitch, 1), offs[al[1]] + p - al[1]).fill_(True)
        # a stray store of a replay would repeat the bytes the step itself left there and change nothing: every byte of the touched allocations
        # that the call does NOT declare is inverted for the replay (and put back behind it)
        flips = [(views[order.index(b)], (~declared[offs[b]:offs[b] + allocs.by_base[b][2]]).to(torch.uint8) * 255) for b in touched]
        for v, m in flips:
            v.bitwise_xor_(m)
        torch.cuda.synchronize()
        before = torch.cat(views)
        rc = getattr(rec.real, r["name"])(*r["args"], st)
        torch.cuda.synchronize()
        assert rc == 0, (form, rc)
        stray = (torch.cat(views) != before) & ~written
        for v, m in flips:
            v.bitwise_xor_(m)
        if bool(stray.any()):
            at = int(stray.nonzero()[0])
            b = max(x for x in order if offs[x] <= at)
            bad.append((form, allocs.by_base[b][0], at - offs[b], int(stray.sum())))
    print(f"sched-hazards write sets: {len(forms)} forms replayed, {total} bytes watched, stray writes {bad}")
    assert bad == []


# ------------------------------------------------------------------------------------------------ f. the checker sees what it is there for
def _copy(trace):
    out = [dict(r) for r in trace]
    for i, r in enumerate(out):
        r["uid"] = i
    return out


def _first(res):
    assert res.findings, "the mutated trace has no finding"
    return res.findings[0]


def _wgrad3x3(rec, trace, side):
    """side-stream 3x3 weight gradients of step 1: [(trace position, record)]"""
    out = []
    for i, r in enumerate(trace):
        if r["op"] == "launch" and r["name"] == "conv2d_wgrad" and r["stream"] == side and r["step"] == 1:
            if sh.named_args(rec.directions, "conv2d_wgrad", r["args"] + (None,))["KH"] == 3:
                out.append((i, r))
    return out


def test_mutated_schedules_are_caught(rec, compact_default):
    """the recorded default-schedule trace of the compact net, mutated on the host (nothing runs on the GPU again)"""
    net, trace, allocs = compact_default
    side, main = net.plan.side().cuda_stream, torch.cuda.current_stream().cuda_stream
    assert sh.analyse(_copy(trace), allocs).findings == []

    # 1. the fork, or the arm / wait pair, in front of one 3x3 weight gradient is gone
    i, prev = next((i, trace[i - 1]) for i, r in _wgrad3x3(rec, trace, side) if trace[i - 1]["op"] in ("fork", "fwait"))
    drop = {i - 1}
    if prev["op"] == "fwait":
        drop.add(max(j for j in range(i - 1) if trace[j]["op"] == "arm" and trace[j]["ev"] == prev["ev"]))
    f = _first(sh.analyse([x for j, x in enumerate(_copy(trace)) if j not in drop], allocs))
    assert f.later["uid"] == i and f.later["name"] == "conv2d_wgrad" and f.earlier["stream"] == main, (prev["op"], f)

    # 2. a deferred slab reduce moves ahead of the fork that follows its pw_bwd
    t = _copy(trace)
    top, pick = -1, None
    for i, r in enumerate(t):
        if r["op"] == "launch" and r["step"] == 1 and r.get("entry") and r["entry"][0] == "bwd":
            if r["name"] == "wgrad_reduce" and r["entry"][1] < top and pick is None:
                pick = i
            top = max(top, r["entry"][1])
    ws = sh.named_args(rec.directions, "wgrad_reduce", t[pick]["args"] + (None,))["ws"]
    prod = [i for i, r in enumerate(t) if r["op"] == "launch" and r["name"] == "pw_bwd" and r["step"] == 1 and
            sh.named_args(rec.directions, "pw_bwd", r["args"] + (None,))["ws"] == ws]
    assert len(prod) == 1 and prod[0] < pick
    moved = t.pop(pick)
    t.insert(prod[0] + 1, moved)
    res = sh.analyse(t, allocs)
    f = _first(res)
    assert f.later["uid"] == pick and f.later["name"] == "wgrad_reduce", f
    assert [x for x in res.findings if x.later["uid"] == pick and x.earlier["uid"] == prod[0] and x.label.startswith("RAW")], res.findings[:4]

    # 3. a side-stream weight gradient is re-labelled as main-stream and keeps its workspace pointer
    t = _copy(trace)
    pick = _wgrad3x3(rec, trace, side)[-1][0]
    t[pick]["stream"] = main
    f = _first(sh.analyse(t, allocs))
    assert pick in (f.later["uid"], f.earlier["uid"]) and f.later["name"] == "conv2d_wgrad", f

    # 4. the final side -> main fork of step 1 is gone: a weight gradient against the optimizer step (or the next step's forward)
    last = max(i for i, r in enumerate(trace) if r["op"] == "fork" and r["step"] == 1 and r["src"] == side and r["dst"] == main)
    res = sh.analyse([x for j, x in enumerate(_copy(trace)) if j != last], allocs)
    wg = ("conv2d_wgrad", "conv2d_wgrad_bnapply", "wgrad_reduce")
    hit = [f for f in res.findings if f.earlier["name"] in wg and f.earlier["stream"] == side and
           (f.later["name"].startswith("adam_step") or f.later["step"] == 2)]
    assert hit, res.findings[:5]
    print(f"sched-hazards mutations: dropped fork / arm+wait, early reduce, re-labelled weight gradient, dropped final fork "
          f"({len(res.findings)} findings, first {res.findings[0]}) all caught")
