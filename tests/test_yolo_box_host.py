"""Box loss of the YOLO head, host half (no GPU): include/mdcv_box.h against the built libmdcv_box.so, the entries' argument checks, the
keywords of Darknet / YOLOLayer / train() and the CLI flags."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from mdcv import _lib
from mdcv.yolo import train as T
from mdcv.yolo.models import Darknet, YOLOLayer

GOOD = dict(dtype=0, ldc=32, ldd=32, Cpad=32, B=2, T=3, A=3, C=4, Gh=13, Gw=13, thresh=0.5, mode=2, box_loss=1.0, stream=None)


def test_the_header_declares_the_entries_and_the_library_exports_them():
    protos = _lib.parse_header(_lib.BOX_HEADER)
    assert list(protos) == ["mdcv_yolo_box_workspace_bytes", "mdcv_yolo_box_loss", "mdcv_yolo_box_grad"]
    assert not any(set(_lib.parse_header(h)) & set(protos) for h in (_lib.HEADER, _lib.AUG_HEADER, _lib.KPTAUG_HEADER, _lib.CLS_HEADER))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.BOX_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (mdcv_\w+)", out)) == set(protos)                 # the library exports exactly its header
    K, text = _lib.box_lib(), open(_lib.BOX_HEADER).read()
    assert K is _lib.box_lib() and K is not _lib.lib() and int(K.yolo_box_workspace_bytes()) == 16
    assert set(_lib.BOX_MODES) == {"giou", "diou", "ciou"} and all(f"#define MDCV_BOX_{k.upper()} {v}\n" in text for k, v in _lib.BOX_MODES.items())


@pytest.mark.parametrize("entry", ["mdcv_yolo_box_loss", "mdcv_yolo_box_grad"])
def test_every_bad_argument_is_reported_without_a_gpu(entry):
    """host arrays stand in for the device buffers: a bad argument returns before anything is dereferenced or launched"""
    names = _lib.parse_header(_lib.BOX_HEADER)[entry][2]
    buf = {n: np.zeros(64, np.float64) for n in names if n not in GOOD}

    def c(**over):
        a = dict(GOOD, **{k: v.ctypes.data for k, v in buf.items()})
        a.update(over)
        return getattr(_lib.box_lib(), entry[5:])(*[a[k] for k in names])
    assert all(c(**{p: None}) == -1 for p in buf if p != "gscale")
    assert c(dtype=2) == -1 and c(dtype=-1) == -1 and c(mode=3) == -1 and c(mode=-1) == -1
    assert all(c(**{n: v}) == -1 for n in ("B", "T", "A", "C", "Gh", "Gw") for v in (0, -3))
    assert c(Gh=4096) == -1 and c(Gw=4096) == -1 and c(A=128, ldc=4096, Cpad=4096, ldd=4096) == -1      # the head's limits
    assert c(ldc=26) == -1 and c(B=1 << 16, T=1 << 15) == -1                      # 3 * (5 + 4) = 27 channels; B * T = 2^31 rows
    if entry.endswith("grad"):
        assert c(Cpad=26) == -1 and c(ldd=31) == -1
    else:
        assert c(box_workspace=buf["box_workspace"].ctypes.data + 4) == -1         # the fp64 accumulators' alignment


def test_models_and_cli_accept_and_store_the_keywords(monkeypatch):
    monkeypatch.chdir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mini"))
    dark = lambda *a, **kw: Darknet("mini_tiny.cfg", 2.0, 1.6, 25.0, 0.1, False, *a, **kw)             # noqa: E731
    layer = lambda **kw: YOLOLayer([[10, 13]], 3, 64, 64, 0.5, "leaky", 2.0, 1.6, 0.1, 25.0, **kw)     # noqa: E731
    heads = lambda n: [m[0] for m in n.module_list if isinstance(m[0], YOLOLayer)]                      # noqa: E731
    for m in [dark(), layer()] + heads(dark()):
        assert (m.box_loss, m.box_mode, m.loss_box, m.box_iou) == (0.0, "ciou", None, None)
    net = dark("fp32", box_loss=0.5, box_mode="giou", cls_loss=0.25)
    assert (net.box_loss, net.box_mode, net.cls_loss) == (0.5, "giou", 0.25) and [(h.box_loss, h.box_mode) for h in heads(net)] == [(0.5, "giou")] * 2
    for make in (dark, layer):
        for kw in (dict(box_mode="siou"), dict(box_loss=1.0, box_mode="iou")):           # unknown, also with box_loss == 0
            with pytest.raises(ValueError, match="box_mode"):
                make(**kw)
    sig = inspect.signature(T.train).parameters
    assert sig["box_loss"].default == 0.0 and sig["box_mode"].default == "ciou"
    opt = T._parser().parse_args(["--model_cfg", "x.cfg"])
    assert opt.box_loss == 0.0 and opt.box_mode == "ciou"
    opt = T._parser().parse_args(["--model_cfg", "x.cfg", "--box_loss", "0.5", "--box_mode", "diou"])
    assert opt.box_loss == 0.5 and opt.box_mode == "diou"
    with pytest.raises(SystemExit):
        T._parser().parse_args(["--model_cfg", "x.cfg", "--box_mode", "siou"])
