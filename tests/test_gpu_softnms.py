"""Soft-NMS (csrc/soft_nms.hip) against its NumPy restatement (tests/helpers/softnms_numpy.py) and, with the hard method,
against the existing entries.

Against float64 a score decayed d times may differ by 2 d 2^-23 relative (per decay an ulp for the rounded weight, the two double exp may
differ in the last place, and one for the product); the reference's own decisions clear four times that (`margin`) at the chosen seeds."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import mcdet_numpy as MC  # noqa: E402
import softnms_numpy as S  # noqa: E402

pytestmark = pytest.mark.gpu
F, NMS, SIGMA, STHRES = np.float32, 0.3, 0.5, 0.05
SIZES = (1, 2, 63, 64, 65, 130, 512, 700)       # the lane edge, the wave edge, two waves, all eight waves, n > top_k (the select runs)
_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731


def _soft(b, s, method, top_k=200, classes=None, nms=NMS, sthres=STHRES):
    from mdcv.yolo.utils.nms import soft_nms
    keep, out = soft_nms(_dev(b), _dev(s), nms, top_k, method, SIGMA, sthres, None if classes is None else _dev(classes))
    return keep.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("top_k", (1, 200, 512))
@pytest.mark.parametrize("n", SIZES)
def test_soft_nms_equals_the_restatement(n, top_k):
    from mdcv.yolo.utils.nms import nms
    b, s = S.scene(n, 1)
    cls = np.random.default_rng(n).choice(np.array([-3, 0, 70000]), n)
    for classes in (None, cls):                                                             # hard: the existing entries, ==
        keep, out = _soft(b, s, "hard", top_k, classes)
        want = nms(_dev(b), _dev(s), NMS, top_k, classes=None if classes is None else _dev(classes)).cpu().numpy()
        assert np.array_equal(keep, want) and np.array_equal(out.view(np.uint32), s[want].view(np.uint32))
    (keep, out), (want, wout, _, _) = _soft(b, s, "linear", top_k), S.soft_nms(b, s, None, "linear", NMS, SIGMA, STHRES, top_k, F)    # linear, float32: ==
    assert np.array_equal(keep, want) and np.array_equal(out.view(np.uint32), wout.view(np.uint32))
    for method in ("linear", "gaussian"):                                                   # float64: the order ==, the scores to 2 d 2^-23
        want, wout, d, margin = S.soft_nms(b, s, None, method, NMS, SIGMA, STHRES, top_k, np.float64)
        assert margin > 4, (method, margin)
        keep, out = _soft(b, s, method, top_k)
        err = np.abs(out.astype(np.float64) - wout) / wout
        assert np.array_equal(keep, want) and (err <= 2 * d * S.EPS).all()


# a near cone and the far cone inside its box, both confident, and 40 distractors elsewhere
_two_cones = lambda: (np.concatenate([np.array([[100, 100, 160, 180], [112, 100, 158, 160]], F), S.scene(40, 3)[0] + F(600)]),  # noqa: E731
                      np.concatenate([np.array([0.95, 0.9], F), S.scene(40, 3)[1]]))
NAMED = {
    "equal scores": lambda: (S.scene(130, 4)[0], (np.round(S.scene(130, 4)[1] * 8) / 8).astype(F), None, STHRES),
    "disjoint": lambda: (np.array([[i * 50, 0, i * 50 + 40, 40] for i in range(70)], F), S.scene(70, 5)[1], None, STHRES),
    "identical": lambda: (np.tile(np.array([[10, 10, 50, 60]], F), (66, 1)), S.scene(66, 6)[1], None, STHRES),
    "zero area": lambda: (np.concatenate([np.array([[30, 30, 30, 30]] * 2, F), S.scene(30, 7)[0]]), S.scene(32, 7)[1], None, STHRES),
    "classes": lambda: (*S.scene(200, 8), np.random.default_rng(8).choice(np.array([0, 2]), 200), STHRES),      # class 1 is empty
    "stops midway": lambda: (*S.scene(200, 9), None, 0.4),
    "two cones": lambda: (*_two_cones(), None, 0.3),
}


@pytest.mark.parametrize("name", NAMED)
def test_named_cases(name):
    b, s, classes, sthres = NAMED[name]()
    got = {}
    for method in ("hard", "linear", "gaussian"):
        keep, out = got[method] = _soft(b, s, method, 200, classes, sthres=sthres)
        want, wout, d, margin = S.soft_nms(b, s, classes, method, NMS, SIGMA, sthres, 200, F if method != "gaussian" else np.float64)
        assert np.array_equal(keep, want), method
        if method != "gaussian":
            assert np.array_equal(out.view(np.uint32), wout.view(np.uint32)), method
        else:
            assert margin > 4 and (np.abs(out - wout) <= 2 * d * S.EPS * wout).all()
    (keep, out), (gk, go), hk = got["linear"], got["gaussian"], got["hard"][0]
    assert {                                            # what each case is there for
        "disjoint": lambda: np.array_equal(keep, np.argsort(S.keys(s, np.arange(70)))[::-1]) and np.array_equal(out, s[keep]),   # the sort
        "identical": lambda: len(keep) == 1 and len(gk) > 1,                                # weight 0: the rest ends at score_thres
        "zero area": lambda: all(o[k == 0] == s[0] and o[k == 1] == s[1] for k, o in (got["linear"], got["gaussian"])) and np.isin([0, 1], hk).sum() == 1,
        "stops midway": lambda: 0 < len(keep) < 200 and out.min() > 0.4,
        "two cones": lambda: 1 in keep and 1 in gk and 1 not in hk and 0 in hk,             # the re-ordering matters: hard loses the far cone
    }.get(name, lambda: True)()


@pytest.mark.parametrize("class_aware", (False, True))
@pytest.mark.parametrize("case", (0, 1))
def test_detect_postprocess(case, class_aware, monkeypatch):
    """B = 3 with an image without a candidate, and B = 1; every output tensor, `correct` and the stats included"""
    from mdcv import _lib
    from mdcv.yolo.postprocess import detect_postprocess
    B, N, C, T, conf, top_k = ((3, 1500, 5, 12, 0.1, 200), (1, 700, 3, 6, 0.1, 512))[case]
    out, tg = MC.build(B, N, C, T, conf, None, 11 + case)
    args = (conf, 0.25, 0.5, 416.0, 416.0, top_k)
    monkeypatch.setitem(_lib.NMS_METHODS, "hard, by the new entry", 0)
    monkeypatch.setattr(_lib, "_softnms", None)
    old = detect_postprocess(_dev(out), _dev(tg), *args, class_aware=class_aware)
    assert _lib._softnms is None                                                            # the defaults never load the library
    new = detect_postprocess(_dev(out), _dev(tg), *args, class_aware=class_aware, nms="hard, by the new entry")
    for f in old.__slots__:
        assert int(old.count.sum()) > 0 and torch.equal(getattr(old, f).view(torch.uint8), getattr(new, f).view(torch.uint8)), f
    det = detect_postprocess(_dev(out), _dev(tg), *args, class_aware=class_aware, nms="linear")
    for b in range(B):
        r = S.postprocess(out[b], tg[b], *args, "linear", SIGMA, conf, class_aware)
        n = r["count"]
        assert int(det.count[b]) == n and (b != B - 1 or B == 1 or n == 0)
        for f in ("index", "cls", "boxes", "prob", "correct"):
            got = getattr(det, f)[b].cpu().numpy()
            assert np.array_equal(got[:n].view(np.uint8), r[f].astype(got.dtype).view(np.uint8)) and not got[n:].any(), (b, f)
        assert np.array_equal(det.stats[b].cpu().numpy().view(np.uint32), r["stats"].view(np.uint32)), (b, det.stats[b], r["stats"])
    assert int(det.count.sum()) > int(old.count.sum()) and det.correct.any()


def test_validate_and_frame_detector_pass_the_keywords_through(monkeypatch):
    from mdcv import _lib
    from mdcv.yolo.detect import FrameDetector
    from mdcv.yolo.models import Darknet
    from mdcv.yolo.validate import validate
    monkeypatch.chdir(os.path.join(ROOT, "tests", "golden", "mini"))
    net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32")
    net.load_weights("mini.weights", net.get_start_weight_dim())
    z = np.load(os.path.join(ROOT, "tests", "golden", "mini_darknet.npz"))
    loader = type("Loader", (list,), {"dataset": list(range(len(z["x"])))})([(None, torch.from_numpy(z["x"]), torch.from_numpy(z["targets"]))])
    calls, fn = [], _lib.softnms_lib().detect_post_soft
    monkeypatch.setattr(_lib.softnms_lib(), "detect_post_soft", lambda *a: (calls.append(a[12:14]), fn(*a))[1])
    validate(dataloader=loader, model=net.cuda().eval(), device=torch.device("cuda:0"), nms="linear")
    assert len(list(FrameDetector(net, conf_thres=0.01, nms="gaussian", sigma=0.25).detect_frames([np.full((48, 64, 3), 90, np.uint8)]))) == 1
    assert calls == [(1, 0.5), (2, 0.25)]
