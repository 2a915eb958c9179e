"""Class-aware tile merge, host half (no GPU): include/mdcv_mctiles.h against the built libmdcv_mctiles.so, the entry's argument checks,
the ValueErrors of the `tile_merge` keyword, `pack_frames(classes=)` and the batch plans' layout with and without the class table."""
import os
import re
import subprocess

import numpy as np
import pytest

from mdcv import _lib
from mdcv.yolo import detect as DT
from mdcv.yolo.evaluate import DatasetAP

ENTRY = "mdcv_detect_merge_tiles_mc"
TABLE = np.array([[0, 0, 0, 0], [0, 40, 0, 0], [1, -8, -14, 0]], np.int32)
GOOD = dict(T=3, K=8, B=2, overlap=0.5, contain_thres=0.6, top_k=16, stream=None)


def test_the_header_declares_the_entry_and_the_library_exports_it():
    protos = _lib.parse_header(_lib.MCTILES_HEADER)
    assert list(protos) == [ENTRY]
    others = (_lib.HEADER, _lib.AUG_HEADER, _lib.KPTAUG_HEADER, _lib.CLS_HEADER, _lib.BOX_HEADER, _lib.IGN_HEADER, _lib.MCDET_HEADER)
    assert not any(ENTRY in _lib.parse_header(h) for h in others)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.MCTILES_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (mdcv_\w+)", out)) == {ENTRY}                     # the library exports exactly its header
    base = _lib.parse_header(_lib.HEADER)["mdcv_detect_merge_tiles"][2]
    assert [n for n in protos[ENTRY][2] if n not in ("tile_cls", "out_cls")] == base and _lib.mctiles_lib() is not _lib.lib()


def test_every_bad_argument_is_reported_without_a_gpu():   # host arrays stand in for device buffers: nothing is dereferenced or launched
    names = _lib.parse_header(_lib.MCTILES_HEADER)[ENTRY][2]
    buf = {n: np.zeros(64, np.float64) for n in names if n not in GOOD and n != "tiles_host"}

    def c(table=TABLE, **over):
        a = dict(GOOD, tiles_host=table.ctypes.data, **{k: v.ctypes.data for k, v in buf.items()})
        a.update(over)
        return _lib.mctiles_lib().detect_merge_tiles_mc(*[a[k] for k in names])
    assert "tile_cls" in buf and "out_cls" in buf and len(buf) == 10 and all(c(**{p: None}) == -1 for p in buf) and c(tiles_host=None) == -1
    assert all(c(top_k=v) == -1 for v in (0, -1, 513)) and c(K=513) == -1 and c(B=65536) == -1 and all(c(**{n: -1}) == -1 for n in "TKB")
    for bad in ([[2, 0, 0, 0]], [[-1, 0, 0, 0]], [[1, 0, 0, 0], [0, 0, 0, 0]], [[0, (1 << 24) + 1, 0, 0]], [[0, 0, -(1 << 24) - 1, 0]],
                [[0, 0, 0, 5]], [[0, 0, 0, 0]] * 65):
        assert c(table=np.array(bad, np.int32), T=len(bad)) == -1                 # mdcv_detect_merge_tiles's table rules
    assert c(B=0, T=0) == 0 and c(T=0, tile_cls=None) == 0 and c(K=0, out_cls=None) == 0      # empty shapes: MDCV_OK before any pointer


def test_the_value_errors_of_tile_merge(monkeypatch, tmp_path):
    from mdcv.yolo.models import Darknet
    monkeypatch.chdir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mini"))
    net, d = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32"), str(tmp_path)
    kpt = type("Kpt", (), {"image_size": (80, 80), "num_kpt": 7})()
    det = DT.TiledFrameDetector(net, 1.0, class_aware=True, tile_merge="per_class")
    cone = DT.TiledFrameConeDetector(net, kpt, 1.0, class_aware=True, tile_merge="per_class")
    assert det.class_aware and cone.class_aware and det.tile_merge == cone.tile_merge == "per_class"
    assert not DT.TiledFrameDetector(net, 1.0).class_aware and DT.TiledFrameDetector(net, 1.0).tile_merge == "agnostic"
    for match, make in (
            ("tile_merge=\"per_class\"", lambda: DT.TiledFrameDetector(net, 1.0, class_aware=True)),          # the refusal names the keyword
            ("class_aware=True", lambda: DT.TiledFrameConeDetector(net, kpt, 1.0, tile_merge="per_class")),
            ("class_aware=True", lambda: DT.detect(d, d, net, None, 0.5, 0.25, tiles=True, tile_merge="per_class")),
            ("one of", lambda: DT.TiledFrameDetector(net, 1.0, class_aware=True, tile_merge="classes")),
            ("tiled", lambda: DT.single_img_detect(d, d, "image", net, None, 0.5, 0.25, class_aware=True, tile_merge="per_class")),
            ("tiled", lambda: DT.detect(d, d, net, None, 0.5, 0.25, tile_merge="per_class", class_aware=True))):
        with pytest.raises(ValueError, match=match):
            make()


def test_pack_frames_with_classes():
    R = lambda n, cls: DT.FrameDetections(np.arange(4.0 * n).reshape(n, 4), np.linspace(0.9, 0.1, n, dtype=np.float32), None, 0, None, cls)  # noqa: E731
    results = [R(3, np.array([2, -1, 70000], np.int32)), R(0, np.zeros(0, np.int32)), R(6, np.arange(6, dtype=np.int32))]
    labels = [np.ones((2, 4)), np.zeros((0, 4)), np.ones((1, 4))]
    classes = [np.array([1, 2]), np.zeros(0, np.int64), [4]]
    out = DatasetAP.pack_frames(results, labels, 4, classes=classes)
    assert len(out) == 8 and out[2].tolist() == [3, 0, 4]
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(out, DatasetAP.pack_frames(results, labels, 4)))   # the six, unchanged
    cls, gt_cls = out[6:]
    assert cls.dtype == gt_cls.dtype == np.int32 and cls.shape == (3, 4) and gt_cls.shape == (3, 2)
    assert cls.tolist() == [[2, -1, 70000, 0], [0, 0, 0, 0], [0, 1, 2, 3]] and gt_cls.tolist() == [[1, 2], [0, 0], [4, 0]]
    for res, bad in ((results, classes[:2]), (results, [[1], [], [4]]), (results, [np.array([1.0, 2.0]), [], [4]]), ([R(3, None)] + results[1:], classes)):
        with pytest.raises(ValueError, match="classes"):                          # a frame short, a row short, not integers, a result with cls None
            DatasetAP.pack_frames(res, labels, 4, classes=bad)


@pytest.mark.parametrize("tiled", [False, True])
def test_the_plans_move_no_byte_without_class_aware(tiled):
    sizes, K = [(120, 90), (200, 150), (64, 64)], 200
    for aware in (False, True):
        kw = dict(class_aware=True) if aware else {}
        p = DT.TiledBatchPlan(sizes, 64, 64, K, [1.0] * 3, **kw) if tiled else DT.BatchPlan(sizes, 64, 64, K, **kw)
        chain = [("fb_off", 3 * K * 32), ("rect_off", 3 * K * 16), ("prob_off", 3 * K * 4), ("count_off", 12), ("skip_off", 12)]
        at = p.in_bytes
        for name, size in chain + [("cls_off", 3 * K * 4)] * aware + [("src_off", 3 * K * 8)] * tiled:
            assert getattr(p, name) == at, name
            at = DT._align(at + size)
        assert p.nbytes == at and (aware or p.cls_off is None)
