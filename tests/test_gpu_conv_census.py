"""-m gpu: production is a subset of exact.  tests/test_gpu_conv_exact.py compares every convolution kernel family with `==`, case by case, and records
in its ledger (helpers/conv_census_ledger.py) which template instantiation each case launched.  Here the production plans run ONE ordinary step
inside the in-library profiler (helpers/kernel_census.py) and every convolution instantiation they launch must be in the union of the ledger's sets
(or on its WAIVED list): an instantiation a plan spends its time in and no exact case reaches fails here, with the launch that needs covering.

No CPU reference is involved: a plan costs its model build, a warm step and a profiled step.  docs/conv_census.md is the bf16 table these tests print
(MDCV_CENSUS_DOC=<path> writes it)."""
import collections
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
sys.path.insert(0, os.path.dirname(HERE))
import kernel_census as KC  # noqa: E402
import conv_census_ledger as LG  # noqa: E402

# name -> (network, image size, batch, mode, precision).  Closure is asserted for every bf16 plan; the fp32 plans are censused and printed.
PLANS = {
    "yolov3 416 B32 train": ("yolo", 416, 32, "train", "bf16"),            # the benchmark's workload
    "yolov3 800 B4 train": ("yolo", 800, 4, "train", "bf16"),              # the reference cfgs' own size: maps of 25, 50, 100, 200, 400
    "yolov3 608 B8 inference": ("yolo", 608, 8, "inference", "bf16"),      # the joint pipeline's detector
    "tiny 416 B32 train": ("tiny", 416, 32, "train", "bf16"),
    "keypoint 80 B256 train": ("kpt", 80, 256, "train", "bf16"),
    "keypoint 80 B64 inference": ("kpt", 80, 64, "inference", "bf16"),
    "mini yolo fp32 train": ("mini", 64, 2, "train", "fp32"),
    "keypoint 80 B4 fp32 train": ("kpt", 80, 4, "train", "fp32"),
}
BF16_PLANS = [n for n, p in PLANS.items() if p[4] == "bf16"]
FP32_PLANS = [n for n, p in PLANS.items() if p[4] == "fp32"]
BENCH_PLAN = "yolov3 416 B32 train"
_DONE = {}                       # plan name -> Census, filled as the tests run (the table and the WAIVED conditions read it)


class Census:
    def __init__(self, name, counts, plan, step):
        self.name, self.counts, self.plan, self.step = name, counts, plan, step

    def launches_of(self, inst):
        """entry point and geometry of the launches that ran `inst`: engine.run_timed on the same plan (only asked for in a failure message)"""
        from mdcv.engine import run_timed
        out = []
        for lst in (self.plan.fwd, self.plan.bwd if self.plan.has_bwd else []):
            for ent in run_timed(self.plan, lst, kernels=True):
                if any(KC.parse(sym) == inst for sym, _ in ent[3]):
                    out.append(f"{ent[0]}{tuple(a for a in ent[2] if isinstance(a, (int, float)))}")
        return out or ["(not launched from the plan's lists: a side stream or the loss)"]


def _yolo(kind, size, batch, mode, precision, tmp):
    import bench
    from mdcv.yolo.models import Darknet
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        torch.manual_seed(0)
        if kind == "yolo":
            cfg = bench.write_yolo_cfg(tmp, size=size)
        elif kind == "tiny":
            import test_gpu_models as TM
            cfg = TM.write_tiny_cfg(tmp, size, 80)
        else:
            cfg = None
        if cfg is None:
            os.chdir(os.path.join(HERE, "golden", "mini"))
            net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision=precision)
        else:
            net = Darknet(cfg, 2.0, 1.6, 25.0, 0.1, True, precision=precision)
    finally:
        os.chdir(cwd)
    g = torch.Generator().manual_seed(1000)
    x = torch.rand(batch, 3, size, size, generator=g).cuda()
    if mode == "train":
        net = net.cuda().train()
        tg = bench.synth_targets(batch, 16, g).cuda()

        def step():
            out = net(x, tg)
            out[0].sum().backward()
    else:
        net = net.cuda().eval()

        def step():
            with torch.no_grad():
                net(x)
    return net, step


def _kpt(size, batch, mode, precision):
    from mdcv.rektnet.keypoint_net import KeypointNet
    from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss
    torch.manual_seed(0)
    kp = KeypointNet(7, (size, size), precision=precision).cuda()
    g = torch.Generator().manual_seed(0)
    x = torch.rand(batch, 3, size, size, generator=g).cuda()
    if mode == "train":
        kp = kp.train()
        tp = (torch.rand(batch, 7, 2, generator=g) * ((size - 1) / size)).cuda()
        crit = CrossRatioLoss("l1_softargmax", True, 0.05, 0.05)

        def step():
            hm, pts = kp(x)
            crit(hm, pts, None, tp)[2].backward()
    else:
        kp = kp.eval()

        def step():
            with torch.no_grad():
                kp(x)
    return kp, step


def census(name, tmp):
    """default switches, one warm step, one ordinary step (as training runs it, side streams included: the profiler is process-wide) inside launched()"""
    if name in _DONE:
        return _DONE[name]
    from mdcv import _lib
    kind, size, batch, mode, precision = PLANS[name]
    net, step = _kpt(size, batch, mode, precision) if kind == "kpt" else _yolo(kind, size, batch, mode, precision, tmp)
    step()
    torch.cuda.synchronize()
    with KC.launched(_lib.lib()) as syms:
        step()
    counts = collections.Counter(KC.conv_instantiations(syms))
    plan = [p for p in net._plans.values() if p.has_bwd == (mode == "train")][0]
    _DONE[name] = Census(name, counts, plan, step)
    return _DONE[name]


def table(names):
    """markdown: one row per instantiation -- launch count per plan and the exact cases that cover it"""
    insts = sorted({i for n in names for i in _DONE[n].counts}, key=LG.spell)
    rows = ["| instantiation | " + " | ".join(names) + " | covered by |", "|---|" + "---|" * (len(names) + 1)]
    for i in insts:
        cov = LG.covering(i)
        by = (f"{cov[0]}" + (f" (+{len(cov) - 1})" if len(cov) > 1 else "")) if cov else ("WAIVED" if LG.spell(i) in LG.WAIVED else "**none**")
        rows.append(f"| `{KC.show(i)}` | " + " | ".join(str(_DONE[n].counts.get(i, "")) for n in names) + f" | `{by}` |")
    return "\n".join(rows)


@pytest.mark.parametrize("name", BF16_PLANS)
def test_production_is_a_subset_of_exact(name, tmp_path):
    c = census(name, str(tmp_path))
    print(f"\n{name}: {sum(c.counts.values())} convolution launches, {len(c.counts)} instantiations\n" + table([name]))
    assert c.counts, "the profiler saw no convolution kernel"
    have = LG.union() | {KC.parse(s) for s in LG.WAIVED}
    missing = [i for i in c.counts if i not in have]
    if missing:
        msg = [f"{name}: {len(missing)} of {len(c.counts)} production instantiations are reached by no exact case (tests/test_gpu_conv_exact.py):"]
        for i in missing:
            msg.append(f"  {KC.show(i)}  x{c.counts[i]}\n    parameters {KC.named(i)}\n    launched by " + "; ".join(c.launches_of(i)[:4]))
        msg.append("Add the smallest exact case that reaches each (helpers/conv_exact.py DENSE_CASES) and regenerate the ledger: " + LG.REGENERATE)
        raise AssertionError("\n".join(msg))


@pytest.mark.parametrize("name", FP32_PLANS)
def test_fp32_census_is_printed(name, tmp_path):
    """the fp32 plans: census only (asserting their closure is not part of this file yet)"""
    c = census(name, str(tmp_path))
    assert c.counts
    print(f"\n{name}: {sum(c.counts.values())} convolution launches, {len(c.counts)} instantiations\n" + table([name]))


def test_waived_meets_its_conditions_and_table(tmp_path):
    for n in BF16_PLANS:
        census(n, str(tmp_path))
    bench = _DONE[BENCH_PLAN].counts
    hot = ("mdcv_conv3x3_shift_kernel", "pw_block_kernel", "pw_bwd_kernel", "wgrad3x3_stream_kernel", "wgrad3x3_s2_stream_kernel", "wgrad7x7_stream_kernel")
    waived = {KC.parse(s) for s in LG.WAIVED}
    bad = [KC.show(i) for i in waived if i in bench and i[0] in hot]
    assert not bad, f"WAIVED holds instantiations of the benchmark step's hot families: {bad}"
    distinct = {i for n in BF16_PLANS for i in _DONE[n].counts}
    assert 10 * len(waived) <= len(distinct), f"{len(waived)} waived of {len(distinct)} distinct bf16 production instantiations: more than a tenth"
    for s, why in LG.WAIVED.items():
        assert len(why) == 3 and all(why), f"WAIVED[{s}] names its geometry, its reason and the tolerance test that runs it"
    md = table(BF16_PLANS)
    print("\n" + md)
    if os.environ.get("MDCV_CENSUS_DOC"):
        with open(os.environ["MDCV_CENSUS_DOC"], "w") as f:
            f.write(md + "\n")
