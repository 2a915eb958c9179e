"""Class-aware detection post-processing, host half (no GPU): include/mdcv_mcdet.h against the built libmdcv_mcdet.so, the entries'
argument checks, the ValueErrors of the Python surface and the tiled detectors' refusal."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from mdcv import _lib
from mdcv.yolo import detect as DT, evaluate as EV
from mdcv.yolo.postprocess import detect_postprocess
from mdcv.yolo.utils.nms import nms

POST = dict(B=2, N=300, C=3, T=4, conf_thres=0.5, nms_thres=0.25, iou_thres=0.5, width=416.0, height=416.0, top_k=200, stream=None)


def test_the_header_declares_the_entries_and_the_library_exports_them():
    protos = _lib.parse_header(_lib.MCDET_HEADER)
    assert list(protos) == ["mdcv_detect_post_mc_workspace_bytes", "mdcv_detect_post_mc", "mdcv_nms_mc_workspace_bytes", "mdcv_nms_mc"]
    others = (_lib.HEADER, _lib.AUG_HEADER, _lib.KPTAUG_HEADER, _lib.CLS_HEADER, _lib.BOX_HEADER, _lib.IGN_HEADER)
    assert not any(set(_lib.parse_header(h)) & set(protos) for h in others)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.MCDET_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (mdcv_\w+)", out)) == set(protos)                 # the library exports exactly its header
    K, base = _lib.mcdet_lib(), _lib.parse_header(_lib.HEADER)
    assert K is _lib.mcdet_lib() and K is not _lib.lib()
    assert protos["mdcv_detect_post_mc"][1:] == base["mdcv_detect_post"][1:]      # the arguments of mdcv_detect_post, by type and name
    # keys, one 128-byte counter line per image, 16-bit classes (padded to 16 bytes)
    assert int(K.detect_post_mc_workspace_bytes(2, 301)) == 2 * 301 * 8 + 2 * 128 + 1216 and int(K.detect_post_mc_workspace_bytes(0, 5)) == 0


@pytest.mark.parametrize("entry,good", [("mdcv_detect_post_mc", POST), ("mdcv_nms_mc", dict(n=10, overlap=0.5, top_k=200, stream=None))])
def test_every_bad_argument_is_reported_without_a_gpu(entry, good):
    """host arrays stand in for the device buffers: a bad argument returns before anything is dereferenced or launched"""
    names = _lib.parse_header(_lib.MCDET_HEADER)[entry][2]
    buf = {n: np.zeros(64, np.float64) for n in names if n not in good}

    def c(**over):
        a = dict(good, **{k: v.ctypes.data for k, v in buf.items()})
        a.update(over)
        return getattr(_lib.mcdet_lib(), entry[5:])(*[a[k] for k in names])
    assert all(c(**{p: None}) == -1 for p in buf)                                 # targets NULL with T != 0 included
    assert all(c(top_k=v) == -1 for v in (0, -1, 513))
    if entry == "mdcv_nms_mc":
        assert c(n=-1) == -1
    else:
        assert all(c(**{n: v}) == -1 for n in ("B", "N", "C") for v in (0, -3)) and c(T=-1) == -1
        assert c(B=65536) == -1 and c(C=65536) == -1                              # grid.y, and the 16-bit class between the stages


def test_the_value_errors_of_the_python_surface():
    with pytest.raises(ValueError, match="class_aware"):
        detect_postprocess(torch.zeros(1, 8, 5), None, 0.5, 0.25, 0.5, 416, 416, class_aware=True)    # C == 0
    for bad in (torch.zeros(4), torch.zeros(3, dtype=torch.long), torch.zeros(4, 1, dtype=torch.long), torch.zeros(4, dtype=torch.bool)):
        with pytest.raises(ValueError, match="classes"):
            nms(torch.zeros(4, 4), torch.zeros(4), classes=bad)
    with pytest.raises(ValueError, match="class_aware"):
        EV.evaluate_frames([], [], type("Det", (), {"class_aware": False})(), class_aware=True)


def test_the_tiled_detectors_refuse_class_aware(monkeypatch, tmp_path):
    from mdcv.yolo.models import Darknet
    monkeypatch.chdir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mini"))
    net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32")
    kpt = type("Kpt", (), {"image_size": (80, 80), "num_kpt": 7})()
    assert DT.FrameConeDetector(net, kpt, class_aware=True).class_aware and not DT.FrameDetector(net).class_aware
    for make in (lambda: DT.TiledFrameDetector(net, 1.0, class_aware=True), lambda: DT.TiledFrameConeDetector(net, kpt, 1.0, class_aware=True),
                 lambda: DT.detect(str(tmp_path), str(tmp_path), net, None, 0.5, 0.25, tiles=True, class_aware=True)):
        with pytest.raises(ValueError, match="class-agnostic"):
            make()
