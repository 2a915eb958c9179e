"""Soft tile merge, host half (no GPU): header against library, every MDCV_EARG, the ValueErrors of the keywords, the unchanged refusal."""
import os
import re
import subprocess

import numpy as np
import pytest

from mdcv import _lib
from mdcv.yolo import detect as DT

ENTRY = "mdcv_detect_merge_tiles_soft"
TABLE = np.array([[0, 0, 0, 0], [0, 40, 0, 0], [1, -8, -14, 0]], np.int32)
GOOD = dict(T=3, K=8, B=2, overlap=0.5, contain_thres=0.6, top_k=16, method=1, sigma=0.5, score_thres=0.1, class_aware=1, stream=None)


def test_the_header_declares_the_entry_and_the_library_exports_it():
    protos = _lib.parse_header(_lib.SOFTTILES_HEADER)
    assert list(protos) == [ENTRY]
    others = (_lib.HEADER, _lib.AUG_HEADER, _lib.KPTAUG_HEADER, _lib.CLS_HEADER, _lib.BOX_HEADER, _lib.IGN_HEADER, _lib.MCDET_HEADER,
              _lib.MCTILES_HEADER, _lib.SOFTNMS_HEADER)
    assert not any(ENTRY in _lib.parse_header(h) for h in others)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SOFTTILES_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (mdcv_\w+)", out)) == {ENTRY}                     # the library exports exactly its header
    (_, types, names), base = protos[ENTRY], _lib.parse_header(_lib.MCTILES_HEADER)["mdcv_detect_merge_tiles_mc"]
    assert names[:17] + names[21:] == base[2] and types[:17] + types[21:] == base[1]          # the merge's arguments around the four new ones
    assert names[17:21] == ["method", "sigma", "score_thres", "class_aware"] and _lib.softtiles_lib() is not _lib.mctiles_lib()


def test_every_bad_argument_is_reported_without_a_gpu():   # host arrays stand in for device buffers: nothing is dereferenced or launched
    names = _lib.parse_header(_lib.SOFTTILES_HEADER)[ENTRY][2]
    buf = {n: np.zeros(64, np.float64) for n in names if n not in GOOD and n != "tiles_host"}

    def c(table=TABLE, **over):
        a = dict(GOOD, tiles_host=table.ctypes.data, **{k: v.ctypes.data for k, v in buf.items()})
        a.update(over)
        return _lib.softtiles_lib().detect_merge_tiles_soft(*[a[k] for k in names])
    assert len(buf) == 10 and all(c(**{p: None}) == -1 for p in buf) and c(tiles_host=None) == -1
    assert all(c(top_k=v) == -1 for v in (0, -1, 513)) and c(K=513) == -1 and c(B=65536) == -1 and all(c(**{n: -1}) == -1 for n in "TKB")
    for bad in ([[2, 0, 0, 0]], [[-1, 0, 0, 0]], [[1, 0, 0, 0], [0, 0, 0, 0]], [[0, (1 << 24) + 1, 0, 0]], [[0, 0, -(1 << 24) - 1, 0]],
                [[0, 0, 0, 5]], [[0, 0, 0, 0]] * 65):
        assert c(table=np.array(bad, np.int32), T=len(bad)) == -1                 # mdcv_detect_merge_tiles's table rules
    assert all(c(method=v) == -1 for v in (-1, 3)) and all(c(method=2, sigma=v) == -1 for v in (0.0, -1.0, float("nan"), float("inf")))
    assert c(score_thres=float("nan")) == -1 and all(c(class_aware=v) == -1 for v in (-1, 2)) and c(B=0, T=0, method=7) == -1
    assert c(B=0, T=0) == 0 and c(T=0, tile_cls=None) == 0 and c(K=0, out_cls=None) == 0      # empty shapes: MDCV_OK before any pointer
    assert c(B=0, T=0, method=1, sigma=-1.0) == 0                                 # sigma belongs to the Gaussian method only


def test_the_value_errors_of_the_soft_merges(monkeypatch, tmp_path):
    from mdcv.yolo.models import Darknet
    monkeypatch.chdir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mini"))
    net, d = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32"), str(tmp_path)
    kpt = type("Kpt", (), {"image_size": (80, 80), "num_kpt": 7})()
    monkeypatch.setattr(_lib, "_softtiles", None)
    assert DT.TiledFrameDetector(net, 1.0).tile_merge == "agnostic" and _lib.TILE_MERGES[2:] == ("soft", "soft_per_class")
    soft = DT.TiledFrameDetector(net, 1.0, nms="linear", tile_merge="soft")
    cone = DT.TiledFrameConeDetector(net, kpt, 1.0, nms="gaussian", sigma=0.3, class_aware=True, tile_merge="soft_per_class")
    assert (soft.nms, soft.class_aware, cone.sigma, cone.class_aware, cone.tile_merge) == ("linear", False, 0.3, True, "soft_per_class")
    assert _lib._softtiles is None                                                # building a detector loads nothing either
    for match, make in (
            ("tiled", lambda: DT.detect(d, d, net, None, 0.5, 0.25, nms="linear", tile_merge="soft")),
            ("tiled", lambda: DT.single_img_detect(d, d, "image", net, None, 0.5, 0.25, nms="linear", class_aware=True, tile_merge="soft_per_class")),
            ("nms=\"linear\"", lambda: DT.TiledFrameDetector(net, 1.0, tile_merge="soft")),
            ("nms=\"linear\"", lambda: DT.detect(d, d, net, None, 0.5, 0.25, tiles=True, class_aware=True, tile_merge="soft_per_class")),
            ("class_aware=True", lambda: DT.TiledFrameConeDetector(net, kpt, 1.0, nms="linear", tile_merge="soft_per_class")),
            ("class_aware=False", lambda: DT.TiledFrameDetector(net, 1.0, nms="linear", class_aware=True, tile_merge="soft")),
            ("cross-tile merge.*tile_merge=\"soft\"", lambda: DT.TiledFrameDetector(net, 1.0, nms="linear")),         # the default refusal stays
            ("cross-tile merge", lambda: DT.TiledFrameDetector(net, 1.0, nms="gaussian", class_aware=True, tile_merge="per_class")),
            ("sigma", lambda: DT.TiledFrameDetector(net, 1.0, nms="gaussian", sigma=0.0, tile_merge="soft"))):
        with pytest.raises(ValueError, match=match):
            make()
