"""Class-aware detection post-processing (csrc/detect_mc.hip) against its NumPy restatement, compared with `==`."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import mcdet_numpy as MC  # noqa: E402

pytestmark = pytest.mark.gpu
NMS, IOU, SPAN = 0.25, 0.5, 416.0
# (B, N, C, T, conf_thres, score quantum, top_k), seed
CASES = [((3, 200, 1, 4, 0.3, None, 200), 1), ((4, 1500, 5, 12, 0.1, 1 / 64, 200), 2), ((2, 2100, 20, 30, 0.05, 1 / 16, 512), 3),
         ((2, 1100, 80, 8, 0.2, None, 64), 4), ((2, 700, 2, 6, 0.1, 1 / 64, 200), 5)]


_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731


@functools.lru_cache(None)
def _case(i):
    (B, N, C, T, conf, quant, top_k), seed = CASES[i]
    out, tg = MC.build(B, N, C, T, conf, quant, seed, SPAN)
    return out, tg, [MC.restate(out[b], tg[b], conf, NMS, IOU, SPAN, SPAN, top_k) for b in range(B)]


@functools.lru_cache(None)
def _inputs_reach_every_seam():
    refs = [(r, CASES[i][0][6]) for i in range(len(CASES)) for r in _case(i)[2]]
    lens = np.concatenate([r["seg_len"] for r, _ in refs])
    assert lens.max() > 64 and lens.min() == 1 and max(len(r["seg_len"]) for r, _ in refs) > 16        # more classes present than waves
    assert any(((r["seg_start"] % 64 != 0) & (r["seg_len"] > 1)).any() for r, _ in refs)                # a segment starts inside a word
    assert any(r["n_cand"] == 0 for r, _ in refs) and any(0 < r["n_cand"] < k for r, k in refs) and any(r["n_cand"] > k for r, k in refs)
    assert any(r["conf_only"] > 0 for r, _ in refs) and any(r["cross_keep"] for r, _ in refs) and any(r["wrong_class"] for r, _ in refs)
    assert any(r["stats"][3] > 0 and 0 < r["correct"].sum() < r["count"] for r, _ in refs)
    return True


def _same(det, refs, labelled=True):
    for b, r in enumerate(refs):
        n = r["count"]
        assert int(det.count[b]) == n
        for f in ("index", "cls", "boxes", "prob"):
            got = getattr(det, f)[b].cpu().numpy()
            bits = np.uint32 if got.dtype == np.float32 else got.dtype
            assert np.array_equal(got[:n].view(bits), r[f].astype(got.dtype).view(bits)) and not got[n:].any(), (b, f)    # zeros past count
        want_c, want_s = (r["correct"], r["stats"]) if labelled else (np.zeros(n, np.uint8), np.zeros(4, np.float32))
        assert np.array_equal(det.correct[b].cpu().numpy()[:n], want_c) and not det.correct[b, n:].any(), b
        assert np.array_equal(det.stats[b].cpu().numpy().view(np.uint32), want_s.view(np.uint32)), (b, det.stats[b], want_s)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_class_aware_postprocess_equals_the_restatement(i):
    from mdcv.yolo.postprocess import detect_postprocess
    assert _inputs_reach_every_seam()
    (out, tg, refs), conf, top_k = _case(i), CASES[i][0][4], CASES[i][0][6]
    _same(detect_postprocess(_dev(out), _dev(tg), conf, NMS, IOU, SPAN, SPAN, top_k, class_aware=True), refs)
    _same(detect_postprocess(_dev(out), None, conf, NMS, IOU, SPAN, SPAN, top_k, class_aware=True), refs, labelled=False)


def test_one_class_with_unit_class_words_is_the_class_agnostic_path():
    from mdcv.yolo.postprocess import detect_postprocess
    out, tg = _case(0)[0].copy(), _case(0)[1]
    out[..., 5] = 1.0
    a = detect_postprocess(_dev(out), _dev(tg), 0.3, NMS, IOU, SPAN, SPAN, class_aware=True)
    b = detect_postprocess(_dev(out), _dev(tg), 0.3, NMS, IOU, SPAN, SPAN)
    for f in a.__slots__:
        assert int(b.count.sum()) > 0 and torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)), f


def test_nms_with_classes_equals_the_per_class_oracle():
    from mdcv.yolo.utils.nms import nms
    rng, n = np.random.default_rng(7), 700
    c = (rng.random((40, 2)) * 300)[rng.integers(0, 40, n)] + rng.standard_normal((n, 2)) * 4
    s = 30 + 10 * rng.random((n, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32)
    scores = (np.round(rng.random(n) * 32) / 32).astype(np.float32)                                    # tied scores
    classes = rng.choice(np.array([-3, 0, 70000]), n, p=[0.6, 0.3, 0.1])
    for top_k, dtype in ((200, np.int64), (512, np.int32)):
        want = MC.select(boxes, scores, classes, np.arange(n), 0.45, top_k)[0]
        assert np.array_equal(nms(_dev(boxes), _dev(scores), 0.45, top_k, classes=_dev(classes.astype(dtype))).cpu().numpy(), want)
    assert len(want) > len(MC.PO.nms(boxes, scores, 0.45, 512))                                        # classes kept boxes apart


def test_validate_and_frame_detector_pass_the_keyword_through(monkeypatch):
    """on the mini cfg: class_aware=True reaches mdcv_detect_post_mc; the default reaches mdcv_detect_post and never loads the new library"""
    from mdcv import _lib
    from mdcv.yolo.detect import FrameDetector
    from mdcv.yolo.models import Darknet
    from mdcv.yolo.validate import validate
    monkeypatch.chdir(os.path.join(ROOT, "tests", "golden", "mini"))
    net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32")
    net.load_weights("mini.weights", net.get_start_weight_dim())
    net = net.cuda().eval()
    z = np.load(os.path.join(ROOT, "tests", "golden", "mini_darknet.npz"))
    frames = [np.full((48, 64, 3), 90, np.uint8), np.full((40, 40, 3), 200, np.uint8)]

    class Loader(list):
        dataset = list(range(len(z["x"])))
    loader = Loader([(None, torch.from_numpy(z["x"]), torch.from_numpy(z["targets"]))])
    calls = []

    def spy(lib, name):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a: (calls.append(name), fn(*a))[1])
    monkeypatch.setattr(_lib, "_mcdet", None)
    spy(_lib.lib(), "detect_post")
    validate(dataloader=loader, model=net, device=torch.device("cuda:0"))
    assert len(list(FrameDetector(net, conf_thres=0.01).detect_frames(frames))) == 2
    assert calls == ["detect_post"] * 2 and _lib._mcdet is None
    spy(_lib.mcdet_lib(), "detect_post_mc")
    validate(dataloader=loader, model=net, device=torch.device("cuda:0"), class_aware=True)
    assert len(list(FrameDetector(net, conf_thres=0.01, class_aware=True).detect_frames(frames))) == 2
    assert calls[2:] == ["detect_post_mc"] * 2
