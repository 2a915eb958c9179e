"""The plan audit's reference alone (no GPU): tests/helpers/plan_audit.py.

Unit decomposition: the units, run on their own float64 outputs with their contributions summed per node, reproduce DarknetOracle's autograd
(loss, parts, every parameter gradient, every intermediate gradient) to float64 round-off on the audit nets.
Bound soundness: a torch emulation with float32 arithmetic and the stores at the named points stays inside the derived bounds, element for
element, at the shapes the GPU test uses; the largest ratios are printed (and recorded in the helper's docstring).
"""
import os

import pytest
import torch

import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import plan_audit as pa  # noqa: E402
import plan_audit_kpt as pk  # noqa: E402
from oracle import rektnet_oracle as ro  # noqa: E402
from oracle import yolo_oracle as yo  # noqa: E402
from test_gpu_models import write_tiny_cfg  # noqa: E402

D = torch.float64
TINY_WIDTHS = (8, 16, 16, 32, 32, 64, 64)


def tiny_targets():
    g = torch.Generator().manual_seed(4)
    t = torch.zeros(2, 4, 5)
    for b in range(2):
        t[b, :b + 1, 1:3] = torch.rand(b + 1, 2, generator=g) * 0.9 + 0.05
        t[b, :b + 1, 3:5] = torch.rand(b + 1, 2, generator=g) * 0.28 + 0.05
    return t


def make_case(name, tmp):
    """-> oracle, graph, float64 params, x, targets"""
    if name == "compact":
        cfg = pa.write_compact_cfg(str(tmp))
        x = torch.rand(3, 3, 128, 160, generator=torch.Generator().manual_seed(1))
        tg = pa.compact_targets()
    else:
        cfg = write_tiny_cfg(str(tmp), 96, 1, widths=TINY_WIDTHS, name="audittiny")
        x = torch.rand(2, 3, 96, 96, generator=torch.Generator().manual_seed(2))
        tg = tiny_targets()
    orc = yo.DarknetOracle(cfg, anchors=yo.VANILLA_ANCHORS)
    params = pa.oracle_params(orc, 5)
    return orc, pa.Graph(orc.layers), params, x, tg


@pytest.fixture(scope="module", params=["compact", "tiny"])
def case(request, tmp_path_factory):
    return (request.param,) + make_case(request.param, tmp_path_factory.mktemp(request.param))


def test_graph_of_the_compact_cfg(case):
    name, orc, graph, *_ = case
    if name != "compact":
        assert [u.kind for u in graph.units].count("MaxPool") == 6 and not graph.fused_sections()
        return
    assert graph.fused_sections() == [3, 7, 10, 14, 22]                 # every pair but 17-19, whose 3x3 conv the route at 31 reads too
    kinds = [u.kind for u in graph.units]
    assert kinds.count("Shortcut") == 1 and kinds.count("Concat") == 2 and kinds.count("Upsample") == 2 and kinds.count("YoloHead") == 3
    assert sorted(len(v) for v in graph.consumers.values()).count(2) >= 6


def test_units_on_their_own_outputs_reproduce_the_oracle(case):
    name, orc, graph, params, x, tg = case
    torch.manual_seed(0)
    orc.params = {k: v.clone().requires_grad_("running" not in k) for k, v in params.items()}
    orc.keep_outs = True
    ref = orc.forward(x.to(D), tg)
    ref[0].sum().backward()
    tens = pa.decompose_darknet(graph, params, x.to(D), tg, pa.hyper_of(orc))
    worst = {}

    def rel(tag, got, want):
        scale = float(want.abs().max())
        e = float((got - want).abs().max()) / (scale if scale > 0 else 1.0)
        worst[tag] = max(worst.get(tag, 0.0), e)
    rel("loss", tens.out7[0], ref[0].detach())
    rel("parts", tens.out7[1:], torch.stack([r.detach() for r in ref[1:]]))
    for k, p in orc.params.items():
        if "running" not in k:
            rel("parameter gradients", tens.pgrad[k], p.grad)
    n = 0
    for u in graph.units:
        if u.out is None:
            continue
        o = orc.last_outs[u.out]
        rel("activations", tens.act[u.out], o.detach())
        if o.grad is not None:
            rel("intermediate gradients", tens.grad[u.out], o.grad)
            n += 1
    print(f"plan audit decomposition vs DarknetOracle ({name}), largest error relative to the tensor's maximum:", worst)
    assert n >= 20 and set(worst) == {"loss", "parts", "parameter gradients", "activations", "intermediate gradients"}
    assert all(v <= 1e-12 for v in worst.values()), worst


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_emulated_plan_stays_inside_the_derived_bounds(case, bf16):
    name, orc, graph, params, x, tg = case
    P = pa.Prec(bf16)
    hyper = pa.hyper_of(orc)
    tens = pa.emulate_darknet(P, graph, params, x, tg, hyper)
    rep = pa.Report()
    pa.audit_darknet(P, graph, params, tens, tg, hyper, rep)
    w = rep.worst_by_kind()
    print(f"plan audit emulation / bound ({name}, {'bf16' if bf16 else 'fp32'}):",
          {f"{k[0]}.{k[1]}": round(v, 4) for k, v in sorted(w.items())})
    rep.assert_clean(f"emulation of {name}")
    assert len(rep.rows) > 5 * len(graph.units) // 2


# ------------------------------------------------------------------------------------------------ KeypointNet
def test_keypoint_units_on_their_own_outputs_reproduce_the_oracle():
    """loss, heat-map, points, every parameter gradient and the gradient of every node (a0..a4, the blocks' mids) to float64 round-off.  The oracle's
    keypoint_forward keeps no intermediate, so the forward is rebuilt here from its own pieces (ro._bn, the convs of ro.res_block) with
    retain_grad() on every node, and pinned to ro.res_block / ro.keypoint_forward bit for bit."""
    import torch.nn.functional as F
    sd = pk.keypoint_state(3)
    x, tpts = pk.keypoint_batch()
    T = pk.run_keypoint(pa.Prec(False), sd, x, pk.loss_grad(tpts), emulate=False)
    leaf = {k: v.clone().requires_grad_("running" not in k) for k, v in sd.items()}
    nodes = {}

    def keep(name, t):
        t.retain_grad()
        nodes[name] = t
        return t
    a = keep("a0", F.relu(ro._bn(F.conv2d(x.to(D), leaf["conv.weight"], leaf["conv.bias"], padding=3), leaf, "bn", True)))
    for r in range(1, 5):
        p = f"res{r}"
        mid = keep(f"m{r}", F.relu(ro._bn(F.conv2d(a, leaf[f"{p}.conv1.weight"], leaf[f"{p}.conv1.bias"], padding=2, dilation=2), leaf, f"{p}.bn1", True)))
        main = ro._bn(F.conv2d(mid, leaf[f"{p}.conv2.weight"], leaf[f"{p}.conv2.bias"], padding=1), leaf, f"{p}.bn2", True)
        side = ro._bn(F.conv2d(a, leaf[f"{p}.shortcut_conv.weight"], leaf[f"{p}.shortcut_conv.bias"]), leaf, f"{p}.shortcut_bn", True)
        out = F.relu(side + main)
        assert torch.equal(out, ro.res_block(a, leaf, p, True))
        a = keep(f"a{r}", out)
    hm, pts = pk.hr.softargmax(F.conv2d(a, leaf["out.weight"], leaf["out.bias"]), D)
    hm0, pts0 = ro.keypoint_forward(x.to(D), leaf, train=True)
    assert torch.equal(hm, hm0) and torch.equal(pts, pts0)
    loss = ro.cross_ratio_loss(hm, pts, None, tpts.to(D), "l1_softargmax", True, 0.05, 0.05)[2]
    loss.backward()
    own = ro.cross_ratio_loss(T.hm, T.pts, None, tpts.to(D), "l1_softargmax", True, 0.05, 0.05)[2]
    worst = {"loss": abs(float(own) - float(loss.detach())) / abs(float(loss.detach())),
             "pts": float((T.pts - pts.detach()).abs().max()), "hm": float((T.hm - hm.detach()).abs().max() / hm.detach().max())}
    for k, v in leaf.items():
        if "running" in k:
            continue
        want = v.grad if v.grad is not None else torch.zeros_like(v)
        scale = float(want.abs().max())
        tag = "bias gradients in front of BatchNorm" if (k.endswith("bias") and "bn" not in k and not k.startswith("out")) else "parameter gradients"
        if k == "out.bias":                 # softmax is shift invariant: the head's bias gradient is a sum that cancels to round-off of its terms
            scale = float(T.dlg.abs().sum((0, 2, 3)).max())
        e = float((T.pgrad[k] - want).abs().max()) / (scale if tag == "parameter gradients" and scale > 0 else 1.0)
        worst[tag] = max(worst.get(tag, 0.0), e)
    assert set(nodes) == set(T.grad) and len(nodes) == 9
    for k, t in nodes.items():
        worst["activations"] = max(worst.get("activations", 0.0), float((T.act[k] - t.detach()).abs().max() / t.detach().abs().max()))
        worst["intermediate gradients"] = max(worst.get("intermediate gradients", 0.0), float((T.grad[k] - t.grad).abs().max() / t.grad.abs().max()))
    print("plan audit decomposition vs the RektNet oracle, largest error relative to the tensor's maximum:", worst)
    assert len(worst) == 7 and all(v <= 1e-12 for v in worst.values()), worst


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_emulated_keypoint_plan_stays_inside_the_derived_bounds(bf16):
    P = pa.Prec(bf16)
    sd = pk.keypoint_state(3)
    x, tpts = pk.keypoint_batch()
    T = pk.run_keypoint(P, sd, x, pk.loss_grad(tpts), emulate=True)
    rep = pa.Report()
    pk.audit_keypoint(P, sd, T, rep)
    w = {f"{k[0]}.{k[1]}": v for k, v in rep.worst_by_kind().items()}
    print(f"plan audit emulation / bound (KeypointNet, {'bf16' if bf16 else 'fp32'}):", {k: round(v, 4) for k, v in sorted(w.items())})
    rep.assert_clean("emulation of KeypointNet")
    assert len(rep.rows) > 100
