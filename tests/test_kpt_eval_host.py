"""Key-point validation, host half (no GPU): the refusals of mdcv_kpt_eval_rows, which all come before any launch, and the host arithmetic
of KeypointEvaluator.losses() / .distances() on rows taken from tests/golden/kpt_eval.npz, against what the reference's own statements
produced (eval_model's `+= .item()` / `/ batch_num`, utils.calculate_mean_distance), exactly."""
import os

import numpy as np
import pytest
import torch

from mdcv import _lib
from mdcv.rektnet import KeypointEvaluator, eval_model, print_kpt_L2_distance  # noqa: F401
from mdcv.rektnet import evaluate as E

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOSS_TYPES = ("l2_softargmax", "l2_heatmap", "l1_softargmax")
EARG = -1


def test_every_refusal_comes_back_as_earg_without_a_device():
    """Host buffers stand for the device ones: a refused call touches none of them.  A call that passes goes on to its launch: with a GPU
    it returns 0 on real device copies, without one it fails with HIP's own error code, which is not MDCV_EARG (as in
    tests/test_framecache_host.py)."""
    L = _lib.lib()
    gpu = torch.cuda.is_available()
    B, H, W = 3, 5, 7
    keep = []

    def device(a):
        if not gpu:
            return a.ctypes.data
        keep.append(torch.from_numpy(a).cuda())
        return keep[-1].data_ptr()

    hm, thm = device(np.zeros((B, 7, H, W), np.float32)), device(np.zeros((B, 7, H, W), np.float32))
    pts, tpts = device(np.zeros((B, 7, 2), np.float32)), device(np.ones((B, 7, 2), np.float32))
    raw = np.zeros(B * E.ROW + 8, np.float32)
    raw = raw[(-raw.ctypes.data // 4) % 4:]                           # 16-byte aligned rows
    assert raw.ctypes.data % 16 == 0
    rows = device(raw)
    st = torch.cuda.current_stream().cuda_stream if gpu else None

    def call(hm_=hm, pts_=pts, thm_=thm, tpts_=tpts, B_=B, H_=H, W_=W, lt=1, rows_=rows):
        return L.kpt_eval_rows(hm_, pts_, thm_, tpts_, B_, H_, W_, lt, 1, 0.05, 0.07, 240.0, 240.0, rows_, st)

    bad = dict(null_pts=dict(pts_=None), null_tpts=dict(tpts_=None), null_rows=dict(rows_=None), b_zero=dict(B_=0), b_negative=dict(B_=-1),
               b_65536=dict(B_=65536), loss_type_3=dict(lt=3), loss_type_minus_1=dict(lt=-1), heatmap_null_hm=dict(hm_=None),
               heatmap_null_thm=dict(thm_=None), heatmap_h_zero=dict(H_=0), heatmap_w_zero=dict(W_=0), heatmap_h_negative=dict(H_=-5),
               rows_off_by_4_bytes=dict(rows_=rows + 4), plane_count_past_int=dict(H_=1 << 15, W_=1 << 15))
    for what, kw in bad.items():
        assert call(**kw) == EARG, what
    for lt in (0, 2):                                                 # the point losses refuse the same things, but need no heat-map
        for what in ("null_pts", "null_tpts", "null_rows", "b_zero", "b_65536"):
            assert call(lt=lt, **bad[what]) == EARG, (lt, what)
    passes = dict(heatmap=dict(), points_l2_without_maps=dict(lt=0, hm_=None, thm_=None, H_=0, W_=0),
                  points_l1_without_maps=dict(lt=2, hm_=None, thm_=None, H_=-1, W_=-1))
    for what, kw in passes.items():
        rc = call(**kw)
        assert rc == 0 if gpu else rc != EARG, (what, rc)
    if gpu:
        torch.cuda.synchronize()
    else:
        assert not raw.any()


def _evaluator_with_rows(rows, loss_function=True):
    """an evaluator whose read-back already happened: .losses() / .distances() are host arithmetic on these rows"""
    class _Loss:
        loss_type, include_geo, geo_loss_gamma_horz, geo_loss_gamma_vert = "l1_softargmax", True, 0.05, 0.07
    ev = KeypointEvaluator(torch.nn.Linear(1, 1), _Loss() if loss_function else None, (80, 80))
    ev._host, ev.n = np.asarray(rows, np.float32), len(rows)
    return ev


def test_losses_and_distances_equal_the_reference_statements_exactly():
    z = np.load(os.path.join(G, "kpt_eval.npz"))
    for lt in LOSS_TYPES:
        for geo in (0, 1):
            rows = np.zeros((6, E.ROW), np.float32)
            rows[:, 0:3] = z[f"per::{lt}:{geo}"]
            rows[:, 3:10] = z["dist"]
            ev = _evaluator_with_rows(rows)
            got, want = ev.losses(), z[f"eval::{lt}:{geo}"]
            assert all(type(v) is float for v in got)
            assert got == tuple(want.tolist()), (lt, geo, got, want)
            mean, total, std = ev.distances()
            assert len(mean) == len(std) == 7
            assert all(type(v) is np.float32 for v in mean + std) and type(total) is np.float32
            assert np.array_equal(np.array(mean), z["dist_mean"]) and np.array_equal(np.array(std), z["dist_std"])
            assert total == z["dist_total"]
            assert str(total) == str(z["dist_total"][()])              # what logs/<study_name>.txt holds


def test_edge_cases_of_the_host_arithmetic():
    assert _evaluator_with_rows(np.zeros((1, E.ROW), np.float32)).dist_scale == (240.0, 240.0)
    assert KeypointEvaluator(torch.nn.Linear(1, 1), None, 64).dist_scale == (192.0, 192.0)
    with pytest.raises(ZeroDivisionError):                            # an empty loader, as the reference's 0 / 0
        E.loss_sums(np.zeros((0, E.ROW), np.float32))
    with pytest.raises(ValueError):
        _evaluator_with_rows(np.zeros((2, E.ROW), np.float32), loss_function=False).losses()
    rows = np.zeros((3, E.ROW), np.float32)
    rows[1, 0] = rows[1, 2] = np.nan                                  # one NaN sample poisons the mean, as `+= .item()` does
    loc, geo, tot = _evaluator_with_rows(rows).losses()
    assert np.isnan(loc) and geo == 0.0 and np.isnan(tot)
    # sizes as the default collate hands them over (three [B] tensors) and as SyntheticConeCrops does (one tuple per sample)
    assert E._per_sample_sizes([torch.tensor([60, 61, 62]), torch.tensor([40, 41, 42]), torch.tensor([3, 3, 3])], 3) == [(60, 40), (61, 41), (62, 42)]
    assert E._per_sample_sizes([(80, 80, 3)] * 3, 3) == [(80, 80)] * 3
    with pytest.raises(ValueError):
        E._per_sample_sizes([(80, 80, 3)] * 2, 3)
    with pytest.raises(ValueError):
        KeypointEvaluator(torch.nn.Linear(1, 1), None, 80, chunk=0)
