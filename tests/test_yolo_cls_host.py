"""Class loss of the YOLO head, host half (no GPU): include/mdcv_cls.h against the built libmdcv_cls.so, the entries' argument checks,
the keywords of Darknet / YOLOLayer / train() and the CLI flags."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from mdcv import _lib
from mdcv.yolo import train as T
from mdcv.yolo.models import Darknet, YOLOLayer

MINI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mini")
GOOD = dict(dtype=0, ldc=32, ldd=32, Cpad=32, B=2, T=3, A=3, C=4, Gh=13, Gw=13, thresh=0.5, mode=0, cls_loss=1.0, stream=None)


def test_the_header_declares_the_entries_and_the_library_exports_them():
    protos = _lib.parse_header(_lib.CLS_HEADER)
    assert list(protos) == ["mdcv_yolo_cls_workspace_bytes", "mdcv_yolo_cls_loss", "mdcv_yolo_cls_grad"]
    others = set(_lib.parse_header()) | set(_lib.parse_header(_lib.AUG_HEADER)) | set(_lib.parse_header(_lib.KPTAUG_HEADER))
    assert not others & set(protos)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.CLS_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (mdcv_\w+)", out)) == set(protos)                 # the library exports exactly its header
    K = _lib.cls_lib()
    assert K is _lib.cls_lib() and K is not _lib.lib() and int(K.yolo_cls_workspace_bytes()) == 16
    text = open(_lib.CLS_HEADER).read()
    assert f"#define MDCV_CLS_ERR_WORD {_lib.CLS_ERR_WORD}\n" in text
    assert all(f"#define MDCV_CLS_{k.upper()} {v}\n" in text for k, v in _lib.CLS_MODES.items())


@pytest.mark.parametrize("entry", ["mdcv_yolo_cls_loss", "mdcv_yolo_cls_grad"])
def test_every_bad_argument_is_reported_without_a_gpu(entry):
    """host arrays stand in for the device buffers: a bad argument returns before anything is dereferenced or launched"""
    names = _lib.parse_header(_lib.CLS_HEADER)[entry][2]
    buf = {n: np.zeros(64, np.float64) for n in names if n not in GOOD}

    def c(**over):
        a = dict(GOOD, **{k: v.ctypes.data for k, v in buf.items()})
        a.update(over)
        return getattr(_lib.cls_lib(), entry[5:])(*[a[k] for k in names])
    for p in (n for n in buf if n != "gscale"):
        assert c(**{p: None}) == -1, p
    assert c(dtype=2) == -1 and c(dtype=-1) == -1 and c(mode=2) == -1 and c(mode=-1) == -1
    for n in ("B", "T", "A", "C", "Gh", "Gw"):
        assert c(**{n: 0}) == -1 and c(**{n: -3}) == -1, n
    assert c(Gh=4096) == -1 and c(Gw=4096) == -1 and c(A=128, ldc=4096, Cpad=4096, ldd=4096) == -1      # the head's limits
    assert c(C=4097, ldc=1 << 20, Cpad=1 << 20, ldd=1 << 20) == -1
    assert c(ldc=26) == -1 and c(B=1 << 16, T=1 << 15) == -1                      # 3 * (5 + 4) = 27 channels; B * T = 2^31 rows
    if entry.endswith("grad"):
        assert c(Cpad=26) == -1 and c(ldd=31) == -1
    else:
        assert c(cls_workspace=buf["cls_workspace"].ctypes.data + 4) == -1         # the fp64 accumulator's alignment


def test_models_and_cli_accept_and_store_the_keywords(monkeypatch):
    monkeypatch.chdir(MINI)
    heads = lambda n: [m[0] for m in n.module_list if isinstance(m[0], YOLOLayer)]      # noqa: E731
    net = Darknet("mini_tiny.cfg", 2.0, 1.6, 25.0, 0.1, False)
    assert (net.cls_loss, net.cls_mode, net.loss_cls) == (0.0, "ce", None) and all((h.cls_loss, h.cls_mode) == (0.0, "ce") for h in heads(net))
    net = Darknet("mini_tiny.cfg", 2.0, 1.6, 25.0, 0.1, False, "fp32", cls_loss=0.5, cls_mode="bce")
    assert (net.cls_loss, net.cls_mode) == (0.5, "bce") and [(h.cls_loss, h.cls_mode) for h in heads(net)] == [(0.5, "bce")] * 2
    assert net.get_loss_constant() == [2.0, 1.6, 25.0, 0.1]
    with pytest.raises(TypeError):
        Darknet("mini_tiny.cfg", 2.0, 1.6, 25.0, 0.1, False, "fp32", 0.5)               # keyword-only behind the reference's arguments
    with pytest.raises(ValueError):
        Darknet("mini_tiny.cfg", 2.0, 1.6, 25.0, 0.1, False, cls_mode="focal")
    lay = YOLOLayer([[10, 13]], 3, 64, 64, 0.5, "leaky", 2.0, 1.6, 0.1, 25.0, cls_loss=2.0)
    assert (lay.cls_loss, lay.cls_mode, lay.object_loss, lay.no_object_loss) == (2.0, "ce", 0.1, 25.0)
    sig = inspect.signature(T.train).parameters
    assert sig["cls_loss"].default == 0.0 and sig["cls_mode"].default == "ce"
    opt = T._parser().parse_args(["--model_cfg", "x.cfg"])
    assert opt.cls_loss == 0.0 and opt.cls_mode == "ce"
    opt = T._parser().parse_args(["--model_cfg", "x.cfg", "--cls_loss", "0.5", "--cls_mode", "bce"])
    assert opt.cls_loss == 0.5 and opt.cls_mode == "bce"
    with pytest.raises(SystemExit):
        T._parser().parse_args(["--model_cfg", "x.cfg", "--cls_mode", "focal"])
