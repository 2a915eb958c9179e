"""Soft-NMS, host half (no GPU): header against library, the entries' argument checks, the ValueErrors of the surface, the tiled refusal."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from mdcv import _lib
from mdcv.yolo import detect as DT
from mdcv.yolo.postprocess import detect_postprocess
from mdcv.yolo.utils.nms import nms, soft_nms

POST = dict(B=2, N=300, C=3, T=4, conf_thres=0.5, nms_thres=0.25, iou_thres=0.5, width=416.0, height=416.0, top_k=200, method=1, sigma=0.5,
            score_thres=0.5, class_aware=1, stream=None)
NMS = dict(n=10, method=2, nms_thres=0.5, sigma=0.5, score_thres=0.0, top_k=200, stream=None, classes=None)


def test_the_header_declares_the_entries_and_the_library_exports_them():
    protos = _lib.parse_header(_lib.SOFTNMS_HEADER)
    assert list(protos) == ["mdcv_soft_nms_workspace_bytes", "mdcv_soft_nms", "mdcv_detect_post_soft_workspace_bytes", "mdcv_detect_post_soft"]
    assert not any(set(_lib.parse_header(h)) & set(protos) for h in (_lib.HEADER, _lib.MCDET_HEADER, _lib.MCTILES_HEADER))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SOFTNMS_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (mdcv_\w+)", out)) == set(protos)                 # the library exports exactly its header
    K, (_, types, names), base = _lib.softnms_lib(), protos["mdcv_detect_post_soft"], _lib.parse_header(_lib.HEADER)["mdcv_detect_post"]
    assert names[:12] + names[16:] == base[2] and types[:12] + types[16:] == base[1]     # mdcv_detect_post's arguments around the four new ones
    assert names[12:16] == ["method", "sigma", "score_thres", "class_aware"]
    assert int(K.detect_post_soft_workspace_bytes(2, 301)) == 2 * 301 * 8 + 2 * 128 + 1216 and int(K.soft_nms_workspace_bytes(10)) == 208


@pytest.mark.parametrize("entry,good", [("mdcv_detect_post_soft", POST), ("mdcv_soft_nms", NMS)])
def test_every_bad_argument_is_reported_without_a_gpu(entry, good):
    """host arrays stand in for the device buffers: a bad argument returns before anything is dereferenced or launched"""
    names = _lib.parse_header(_lib.SOFTNMS_HEADER)[entry][2]
    buf = {n: np.zeros(64, np.float64) for n in names if n not in good}

    def c(**over):
        a = dict(good, **{k: v.ctypes.data for k, v in buf.items()})
        a.update(over)
        return getattr(_lib.softnms_lib(), entry[5:])(*[a[k] for k in names])
    assert all(c(**{p: None}) == -1 for p in buf)                                 # targets NULL with T != 0 included
    assert all(c(top_k=v) == -1 for v in (0, -1, 513)) and all(c(method=v) == -1 for v in (-1, 3))
    assert all(c(method=2, sigma=v) == -1 for v in (0.0, -1.0, float("nan"), float("inf"))) and c(score_thres=float("nan")) == -1
    if entry == "mdcv_soft_nms":
        assert c(n=-1) == -1
    else:
        assert all(c(**{n: v}) == -1 for n in ("B", "N") for v in (0, -3)) and c(T=-1) == -1 and c(C=-1) == -1 and c(C=0) == -1
        assert c(B=65536) == -1 and c(C=65536) == -1 and c(class_aware=2) == -1   # grid.y, the 16-bit class between the stages


def test_the_value_errors_of_the_python_surface():
    out, bx, sc = torch.zeros(1, 8, 6), torch.zeros(4, 4), torch.zeros(4)
    for method, sigma in (("soft", 0.5), ("gaussian", 0.0), ("gaussian", float("nan"))):
        for call in (lambda: detect_postprocess(out, None, 0.5, 0.25, 0.5, 416, 416, nms=method, sigma=sigma),
                     lambda: nms(bx, sc, method=method, sigma=sigma), lambda: soft_nms(bx, sc, method=method, sigma=sigma)):
            with pytest.raises(ValueError, match="nms method|sigma"):
                call()
    for kw, what in ((dict(score_thres=float("nan")), "score_thres"), (dict(classes=torch.zeros(3, dtype=torch.long)), "classes")):
        with pytest.raises(ValueError, match=what):
            soft_nms(bx, sc, **kw)


def test_the_tiled_detectors_refuse_a_soft_method(monkeypatch, tmp_path):
    from mdcv.yolo.models import Darknet
    monkeypatch.chdir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mini"))
    net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32")
    kpt = type("Kpt", (), {"image_size": (80, 80), "num_kpt": 7})()
    assert DT.FrameConeDetector(net, kpt, nms="gaussian", sigma=0.3).sigma == 0.3 and DT.FrameDetector(net).nms == "hard"
    for make in (lambda: DT.TiledFrameDetector(net, 1.0, nms="linear"), lambda: DT.TiledFrameConeDetector(net, kpt, 1.0, nms="gaussian"),
                 lambda: DT.detect(str(tmp_path), str(tmp_path), net, None, 0.5, 0.25, tiles=True, nms="linear")):
        with pytest.raises(ValueError, match="cross-tile merge"):
            make()
    with pytest.raises(ValueError, match="nms method"):
        DT.FrameDetector(net, nms="soft")
