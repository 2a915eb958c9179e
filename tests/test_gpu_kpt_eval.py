"""-m gpu: batched RektNet validation.  csrc/kpt_eval.hip (mdcv_kpt_eval_rows) through the C ABI against the float64 references of
tests/helpers/kpt_eval_refs.py (pinned to the reference project's outputs by tests/test_kpt_eval_refs.py), its exact guarantees, the
plumbing of mdcv.rektnet.KeypointEvaluator, and eval_model / print_kpt_L2_distance against the reference's batch-1 loop on the drop-in
classes.

Tolerances, as in tests/test_gpu_heads.py: every ELEMENT of the rows is held to head_refs.bound(e32, scale) = 8 max(e32, 4 u scale) with
e32 the float32 helper's error on that element and scale the element's float64 magnitude; an element whose reference is exactly 0 (geo
without include_geo, the two pad columns) must be exactly 0.  Every comparison prints `[kpt_eval] <tag>: worst err / max(e32, 4 u scale)`
(run with -s); the assertion holds that figure below 8."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mdcv import _lib  # noqa: E402
from mdcv.rektnet import KeypointEvaluator, eval_model, print_kpt_L2_distance  # noqa: E402
from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss  # noqa: E402
from mdcv.rektnet.keypoint_net import KeypointNet  # noqa: E402
from test_gpu_kernels import st  # noqa: E402
from test_gpu_elementwise import P  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import head_refs as hr  # noqa: E402
import kpt_eval_refs as kr  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F64, F32 = torch.float64, torch.float32
SENT = 0x5A5A5A5A
GH, GV = kr.GAMMA
SX, SY = kr.DIST_SCALE
_INPUTS, _REFS = {}, {}


def inputs(B, H, W):
    """hm, pts, thm, tpts on the CPU, one draw per shape; sample 1 has two coincident predicted key points when B > 2"""
    if (B, H, W) not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * B + 10 * H + W)
        pts, tpts = torch.rand(B, 7, 2, generator=g), torch.rand(B, 7, 2, generator=g) * (1 - 1.0 / max(H, W))
        hm = torch.softmax(torch.randn(B, 7, H * W, generator=g) * 2, -1).view(B, 7, H, W)
        thm = torch.softmax(torch.randn(B, 7, H * W, generator=g) * 3, -1).view(B, 7, H, W)
        if B > 2:
            pts[1, 3] = pts[1, 1]
        _INPUTS[(B, H, W)] = (hm, pts, thm, tpts)
    return _INPUTS[(B, H, W)]


def refs(B, H, W, lt, geo):
    """float64 and float32 rows of the case, computed once"""
    key = (B, H, W, lt, geo) if lt == 1 else (B, 0, 0, lt, geo)
    if key not in _REFS:
        hm, pts, thm, tpts = inputs(B, H, W)
        _REFS[key] = tuple(kr.rows(hm, pts, thm, tpts, hr.LOSS_TYPES[lt], geo, GH, GV, SX, SY, d) for d in (F64, F32))
    return _REFS[key]


class Rows:
    """[n, 12] fp32 rows between two sentinel-filled guard bands of 64 words (16-byte alignment kept)"""

    def __init__(self, n, guard=64):
        self.n, self.g = n, guard
        self.raw = torch.full((n * kr.ROW + 2 * guard,), SENT, dtype=torch.int32, device="cuda")
        self.ptr = self.raw.data_ptr() + 4 * guard

    def bits(self):
        return self.raw[self.g:self.g + self.n * kr.ROW].view(self.n, kr.ROW).cpu()

    def vals(self):
        return self.bits().view(torch.float32)

    def guards_intact(self):
        return bool((self.raw[:self.g] == SENT).all()) and bool((self.raw[self.g + self.n * kr.ROW:] == SENT).all())


def run(dev, B, H, W, lt, geo, out=None, maps=True):
    """one call on the device tensors dev = (hm, pts, thm, tpts) -> Rows"""
    L = _lib.lib()
    out = out or Rows(B)
    hm, pts, thm, tpts = dev
    L.check(L.kpt_eval_rows(P(hm) if maps else None, P(pts), P(thm) if maps else None, P(tpts), B, H, W, lt, int(geo), GH, GV, SX, SY, out.ptr,
                            st()), "kpt_eval_rows")
    return out


def compare(tag, got, r64, r32):
    got = got.double()
    assert bool(torch.isfinite(got).all()), f"{tag}: non-finite output"
    e32 = (r32 - r64).abs()
    unit = torch.maximum(e32, 4.0 * hr.U * r64.abs())              # head_refs.bound, element by element
    err = (got - r64).abs()
    exact = unit == 0
    assert bool((err[exact] == 0).all()), f"{tag}: an element whose reference is exactly 0 is not 0"
    ratio = float((err[~exact] / unit[~exact]).max())
    where = int((err / unit.clamp_min(1e-300)).argmax())
    print(f"[kpt_eval] {tag}: worst err / max(e32, 4 u scale) = {ratio:.3f} at row {where // kr.ROW} column {where % kr.ROW}")
    assert bool((err <= 8.0 * unit).all()), f"{tag}: worst err / max(e32, 4 u scale) = {ratio:.3f} (8 allowed)"
    return ratio


CASES = [(B, lt, hw) for B in (1, 2, 64, 65, 257) for lt, hw in ((0, (5, 7)), (2, (5, 7)), (1, (5, 7)), (1, (8, 8)))]


@pytest.mark.parametrize("B,lt,hw", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_rows_against_float64(B, lt, hw):
    """B = 1, 2, on both sides of a wave and of the point kernel's 256-sample block; the three loss types; geo on and off.  5 x 7: an odd
    plane count (245 floats per sample), so the samples' first floats take all four 16-byte phases from i = 1 and both the head and the
    tail are scalar; 8 x 8: every sample aligned.  Guard bands on both sides of the rows stay intact.
    MI355X: worst err / max(e32, 4 u scale) = 0.58 (8 allowed)."""
    H, W = hw
    dev = [t.cuda() for t in inputs(B, H, W)]
    for geo in (False, True):
        out = run(dev, B, H, W, lt, geo)
        torch.cuda.synchronize()
        assert out.guards_intact()
        compare(f"B{B} {hr.LOSS_TYPES[lt]} {H}x{W} geo{int(geo)}", out.vals(), *refs(B, H, W, lt, geo))


@pytest.mark.parametrize("lt", [0, 1, 2], ids=hr.LOSS_TYPES)
def test_rows_at_80x80(lt):
    """the production map size at B = 3: 44 800 floats per sample, 11 198 vector groups, so thread 0 walks its unrolled loop 11 times.
    MI355X: worst err / max(e32, 4 u scale) = 0.32 (8 allowed)."""
    dev = [t.cuda() for t in inputs(3, 80, 80)]
    for geo in (False, True):
        out = run(dev, 3, 80, 80, lt, geo)
        torch.cuda.synchronize()
        assert out.guards_intact()
        compare(f"B3 {hr.LOSS_TYPES[lt]} 80x80 geo{int(geo)}", out.vals(), *refs(3, 80, 80, lt, geo))


@pytest.mark.parametrize("lt", [0, 1, 2], ids=hr.LOSS_TYPES)
def test_a_row_does_not_depend_on_the_batch_around_it(lt):
    """Row i of a B = 257 call equals, bit for bit, the row of a B = 1 call on a COPY of sample i: the copy starts on an allocation
    boundary (phase 0) where sample i of the 5 x 7 batch starts at phase (245 i) % 4.  A second call gives the same bits."""
    B, H, W = 257, 5, 7
    dev = [t.cuda() for t in inputs(B, H, W)]
    whole = run(dev, B, H, W, lt, True)
    again = run(dev, B, H, W, lt, True)
    single = Rows(B)
    L = _lib.lib()
    copies = []
    for i in range(B):
        one = [t[i:i + 1].clone() for t in dev]
        copies.append(one)
        assert one[0].data_ptr() % 16 == 0
        L.check(L.kpt_eval_rows(P(one[0]), P(one[1]), P(one[2]), P(one[3]), 1, H, W, lt, 1, GH, GV, SX, SY, single.ptr + 4 * kr.ROW * i, st()),
                "kpt_eval_rows")
    torch.cuda.synchronize()
    assert {(dev[0].data_ptr() + 4 * 245 * i) % 16 for i in range(B)} == {0, 4, 8, 12}
    assert torch.equal(whole.bits(), again.bits())
    assert torch.equal(whole.bits(), single.bits())
    assert whole.guards_intact() and single.guards_intact()


def test_rows_beyond_the_batch_are_untouched():
    B, H, W = 65, 5, 7
    dev = [t.cuda() for t in inputs(B, H, W)]
    for lt in (0, 1, 2):
        out = Rows(B + 200)
        run(dev, B, H, W, lt, True, out=out)
        torch.cuda.synchronize()
        bits = out.bits()
        assert bool((bits[B:] == SENT).all()) and out.guards_intact()
        assert torch.equal(bits[:B], run(dev, B, H, W, lt, True).bits())


def test_a_nan_target_plane_stays_in_its_sample():
    """prep_label's 0/0 gives an all-NaN target heat-map plane: NaN location and total loss for that sample, as the reference's
    loss; geo, the distances and every other row keep their bits."""
    B, H, W = 64, 5, 7
    hm, pts, thm, tpts = inputs(B, H, W)
    clean = run([t.cuda() for t in (hm, pts, thm, tpts)], B, H, W, 1, True).bits()
    bad = thm.clone()
    bad[3, 2] = float("nan")
    got = run([t.cuda() for t in (hm, pts, bad, tpts)], B, H, W, 1, True)
    torch.cuda.synchronize()
    vals, bits = got.vals(), got.bits()
    assert bool(torch.isnan(vals[3, 0])) and bool(torch.isnan(vals[3, 2]))
    nan = torch.zeros(B, kr.ROW, dtype=torch.bool)
    nan[3, 0] = nan[3, 2] = True
    assert torch.equal(torch.isnan(vals), nan)
    assert torch.equal(bits[~nan], clean[~nan])
    r64 = kr.per_sample(hm, pts, bad, tpts, "l2_heatmap", True, GH, GV, F64)
    assert torch.equal(torch.isnan(r64), nan[:, :3])               # the reference's own NaN pattern


def test_the_point_losses_never_touch_the_heat_maps():
    B = 65
    dev = [t.cuda() for t in inputs(B, 5, 7)]
    for lt in (0, 2):
        with_maps = run(dev, B, 5, 7, lt, True)
        without = run(dev, B, 0, 0, lt, True, maps=False)
        torch.cuda.synchronize()
        assert torch.equal(with_maps.bits(), without.bits()) and without.guards_intact()


# ------------------------------------------------------------------------------------------------ evaluator
def keypoint_net(precision):
    z = np.load(os.path.join(G, "rektnet_net.npz"))
    model = KeypointNet(7, (80, 80), precision=precision)
    model.load_state_dict({k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")})
    return model.cuda()


def samples(n, seed=7):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, 80, 80, generator=g)
    y_hm = torch.softmax(torch.randn(n, 7, 6400, generator=g) * 3, -1).view(n, 7, 80, 80)
    y_pts = torch.rand(n, 7, 2, generator=g) * (79.0 / 80.0)
    return x, y_hm, y_pts


def loader(data, sizes, device=None):
    """batches as the loaders yield them: (x, y_hm, y_pts, names, [h, w, c] as three [B] tensors)"""
    x, y_hm, y_pts = data
    out, lo = [], 0
    for b in sizes:
        s = slice(lo, lo + b)
        t = [v[s] if device is None else v[s].to(device) for v in (x, y_hm, y_pts)]
        shape = [torch.arange(lo, lo + b) + 50, torch.arange(lo, lo + b) + 30, torch.full((b,), 3)]
        out.append((t[0], t[1], t[2], [f"img{i}" for i in range(lo, lo + b)], shape))
        lo += b
    assert lo == x.shape[0]
    return out


@pytest.mark.parametrize("sizes", [[1, 3, 2, 5], [4, 4, 4]], ids=["N11-padded-tail", "N12-full-chunks"])
def test_evaluator_rows_are_the_kernel_on_the_models_chunks(sizes):
    """chunk = 4, fp32: .rows() equals mdcv_kpt_eval_rows called directly on model(x_chunk) for the same chunks (the tail padded with zero
    images, the kernel given the real count), bit for bit; N rows for N samples; the training flag comes back; CPU and device inputs give
    the same bits."""
    n = sum(sizes)
    data = samples(n)
    model = keypoint_net("fp32")
    for loss in (CrossRatioLoss("l2_heatmap", True, GH, GV), CrossRatioLoss("l1_softargmax", True, GH, GV)):
        got = {}
        for where in (None, "cuda"):
            for training in (True, False):
                model.train(training)
                ev = KeypointEvaluator(model, loss, (80, 80), chunk=4)
                for xb, hb, pb, names, shape in loader(data, sizes, where):
                    ev.add(xb, hb, pb, names, shape)
                    assert model.training is training
                rows = ev.rows()
                assert model.training is training and rows.shape == (n, kr.ROW) and rows.is_cuda
                assert ev.names == [f"img{i}" for i in range(n)] and ev.image_sizes() == [(i + 50, i + 30) for i in range(n)]
                got[(where, training)] = rows.clone()
        first = got[(None, True)]
        assert all(torch.equal(first, v) for v in got.values())
        # the same chunks by hand
        direct = Rows(n)
        x, y_hm, y_pts = (t.cuda() for t in data)
        model.eval()
        keep = []
        with torch.no_grad():
            for lo in range(0, n, 4):
                cnt = min(4, n - lo)
                xc = torch.zeros(4, 3, 80, 80, device="cuda")
                xc[:cnt] = x[lo:lo + cnt]
                hm, pts = model(xc)
                dev = (hm, pts.contiguous(), y_hm[lo:lo + cnt].contiguous(), y_pts[lo:lo + cnt].contiguous())
                keep.append(dev)
                lt = 1 if loss.loss_type == "l2_heatmap" else 2
                _lib.lib().check(_lib.lib().kpt_eval_rows(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), cnt, 80, 80, lt, 1, GH, GV, SX, SY,
                                                          direct.ptr + 4 * kr.ROW * lo, st()), "kpt_eval_rows")
        torch.cuda.synchronize()
        assert torch.equal(first.cpu().view(torch.int32), direct.bits()) and direct.guards_intact()
        assert bool(torch.isfinite(first).all()) and bool((first[:, 10:] == 0).all())


def reference_loop(model, batches, loss_function):
    """the statements of the reference's eval_model (RektNet/train_eval.py:117-135) on the drop-in classes, fed batch-1 batches"""
    model.eval()                                                                        # :117
    with torch.no_grad():                                                               # :118
        loss_sums = [0, 0, 0]                                                           # :119
        batch_num = 0                                                                   # :120
        for x_batch, y_hm_batch, y_point_batch, image_name, _ in batches:               # :121
            x_batch = x_batch.to("cuda")                                                # :122
            y_hm_batch = y_hm_batch.to("cuda")                                          # :123
            y_point_batch = y_point_batch.to("cuda")                                    # :124
            output = model(x_batch)                                                     # :125
            loc_loss, geo_loss, loss = loss_function(output[0], output[1], y_hm_batch, y_point_batch)   # :126
            loss_sums[0] += loc_loss.item()                                             # :127
            loss_sums[1] += geo_loss.item()                                             # :128
            loss_sums[2] += loss.item()                                                 # :129
            batch_num += 1                                                              # :131
    return loss_sums[0] / batch_num, loss_sums[1] / batch_num, loss_sums[2] / batch_num  # :133-135


@pytest.mark.parametrize("precision,rel", [("fp32", 1e-4), ("bf16", 3e-2)])
def test_eval_model_agrees_with_the_batch_one_loop(precision, rel, capsys):
    """eval_model fed batches of [1, 3, 2, 5] against the reference's loop at batch 1 over the same 11 samples, to DESIGN 5's figures:
    relative 1e-4 in fp32-kernel mode, 3e-2 in bf16 (one plan at B = 256 against eleven runs of the B = 1 plan: other tiles, other
    summation orders).  The two printed lines and the eval-mode exit are the reference's.
    MI355X: every one of the six figures agreed to the last bit in both modes (relative difference 0)."""
    data = samples(11)
    model = keypoint_net(precision)
    for lt in ("l1_softargmax", "l2_heatmap"):
        loss = CrossRatioLoss(lt, True, GH, GV)
        want = reference_loop(model, loader(data, [1] * 11), loss)
        model.train()
        capsys.readouterr()
        got = eval_model(model, loader(data, [1, 3, 2, 5]), loss, (80, 80))
        lines = capsys.readouterr().out.splitlines()
        assert model.training is False
        assert lines[0] == "\tStarting validation..." and lines[-1].startswith("\tValidation: MSE/Geometric/Total Loss: ")
        assert lines[-1].endswith(f"{round(got[0], 10)}/{round(got[1], 10)}/{round(got[2], 10)}")
        for k, nm in enumerate(("loc", "geo", "total")):
            r = abs(got[k] - want[k]) / abs(want[k])
            print(f"[kpt_eval] eval_model {precision} {lt} {nm}: {got[k]:.8f} vs batch-1 loop {want[k]:.8f} rel {r:.2e}")
            assert r <= rel, (precision, lt, nm, got[k], want[k])
    with pytest.raises(ZeroDivisionError):
        eval_model(model, [], loss, (80, 80))


def test_print_kpt_l2_distance_writes_the_study_file(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    data = samples(11)
    model = keypoint_net("fp32").train()
    keys = ["top", "mid_L_top", "mid_R_top", "mid_L_bot", "mid_R_bot", "bot_L", "bot_R"]
    print_kpt_L2_distance(model, loader(data, [1, 3, 2, 5]), keys, "study7", True, (80, 80))
    out = capsys.readouterr().out
    assert model.training is True
    ev = KeypointEvaluator(model, None, (80, 80))
    for xb, hb, pb, names, shape in loader(data, [11]):
        ev.add(xb, hb, pb)
    mean, total, std = ev.distances()
    assert (tmp_path / "logs" / "study7.txt").read_text() == str(total)
    assert f"Total distance error is: {total}" in out and f"\ttop: {mean[0]}" in out and f"\tbot_R: {std[6]}" in out
    lines = (tmp_path / "logs" / "rektnet_validation.txt").read_text().splitlines()
    d = ev.rows()[:, 3:10].cpu().numpy()
    assert lines == [f"{[i + 30, i + 50]}:{sum(list(d[i]))}" for i in range(11)]
