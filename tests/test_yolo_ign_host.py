"""Prediction-IoU ignore rule of the YOLO head, host half (no GPU): include/mdcv_ign.h against the built libmdcv_ign.so, the entries'
argument checks, the keyword of Darknet / YOLOLayer / train() and the CLI flag."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from mdcv import _lib
from mdcv.yolo import train as T
from mdcv.yolo.models import Darknet, YOLOLayer

GOOD = dict(dtype=0, ldc=32, ldd=32, Cpad=32, B=2, T=3, A=3, C=4, Gh=13, Gw=13, thr=0.5, no_object_loss=25.0, stream=None)


def test_the_header_declares_the_entries_and_the_library_exports_them():
    protos = _lib.parse_header(_lib.IGN_HEADER)
    assert list(protos) == ["mdcv_yolo_ign_workspace_bytes", "mdcv_yolo_ign_rows_per_pass", "mdcv_yolo_ign_loss", "mdcv_yolo_ign_grad"]
    others = (_lib.HEADER, _lib.AUG_HEADER, _lib.KPTAUG_HEADER, _lib.CLS_HEADER, _lib.BOX_HEADER)
    assert not any(set(_lib.parse_header(h)) & set(protos) for h in others)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.IGN_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (mdcv_\w+)", out)) == set(protos)                 # the library exports exactly its header
    K = _lib.ign_lib()
    assert K is _lib.ign_lib() and K is not _lib.lib() and int(K.yolo_ign_rows_per_pass()) >= 64
    # (S, n) in fp64, then four 64-bit words per slab of 256 cells per image: 3 * 13 * 13 = 507 cells are two slabs, 3 * 52 * 52 = 8112 are 32
    assert int(K.yolo_ign_workspace_bytes(2, 3, 13, 13)) == 16 + 2 * 2 * 32 and int(K.yolo_ign_workspace_bytes(32, 3, 52, 52)) == 16 + 32 * 32 * 32


@pytest.mark.parametrize("entry", ["mdcv_yolo_ign_loss", "mdcv_yolo_ign_grad"])
def test_every_bad_argument_is_reported_without_a_gpu(entry):
    """host arrays stand in for the device buffers: a bad argument returns before anything is dereferenced or launched"""
    names = _lib.parse_header(_lib.IGN_HEADER)[entry][2]
    buf = {n: np.zeros(64, np.float64) for n in names if n not in GOOD}

    def c(**over):
        a = dict(GOOD, **{k: v.ctypes.data for k, v in buf.items()})
        a.update(over)
        return getattr(_lib.ign_lib(), entry[5:])(*[a[k] for k in names])
    assert all(c(**{p: None}) == -1 for p in buf if p != "gscale")
    assert c(dtype=2) == -1 and c(dtype=-1) == -1
    assert all(c(**{n: v}) == -1 for n in ("B", "T", "A", "C", "Gh", "Gw") if n in names for v in (0, -3))
    assert c(Gh=4096) == -1 and c(Gw=4096) == -1 and c(A=128, ldc=4096, Cpad=4096, ldd=4096) == -1      # the head's limits
    assert c(B=1 << 20, A=127, Gh=4095, Gw=4095, ldc=4096, Cpad=4096, ldd=4096) == -1                  # 2^20 * 8 319 122 workgroups
    assert c(ign_workspace=buf["ign_workspace"].ctypes.data + 4) == -1                                  # the fp64 sums' alignment
    if entry.endswith("grad"):
        assert c(Cpad=26) == -1 and c(ldd=31) == -1                               # 3 * (5 + 4) = 27 channels
    else:
        assert c(ldc=26) == -1 and c(B=1 << 16, T=1 << 15) == -1                  # B * T = 2^31 rows
        assert all(c(thr=v) == -1 for v in (0.0, 1.0, -0.1, 1.5, float("nan")))


def test_models_and_cli_accept_and_store_the_keyword(monkeypatch):
    monkeypatch.chdir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mini"))
    dark = lambda *a, **kw: Darknet("mini_tiny.cfg", 2.0, 1.6, 25.0, 0.1, False, *a, **kw)             # noqa: E731
    layer = lambda **kw: YOLOLayer([[10, 13]], 3, 64, 64, 0.5, "leaky", 2.0, 1.6, 0.1, 25.0, **kw)     # noqa: E731
    heads = lambda n: [m[0] for m in n.module_list if isinstance(m[0], YOLOLayer)]                      # noqa: E731
    for m in [dark(), layer()] + heads(dark()):
        assert (m.pred_ignore, m.noobj_ignored) == (0.0, None)
    net = dark("fp32", pred_ignore=0.7, box_loss=0.5)
    assert (net.pred_ignore, net.box_loss) == (0.7, 0.5) and [h.pred_ignore for h in heads(net)] == [0.7] * 2
    for make in (dark, layer):
        for v in (1.0, -0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match="pred_ignore"):
                make(pred_ignore=v)
    assert inspect.signature(T.train).parameters["pred_ignore"].default == 0.0
    assert T._parser().parse_args(["--model_cfg", "x.cfg"]).pred_ignore == 0.0
    assert T._parser().parse_args(["--model_cfg", "x.cfg", "--pred_ignore", "0.7"]).pred_ignore == 0.7
