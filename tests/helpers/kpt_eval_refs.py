"""References of csrc/kpt_eval.hip (mdcv_kpt_eval_rows) for tests/test_kpt_eval_refs.py, test_kpt_eval_host.py and test_gpu_kpt_eval.py.

  per_sample   the loss triple of every sample ALONE: head_refs.cross_ratio (oracle.rektnet_oracle.cross_ratio_loss) on the [i:i+1]
               slices, which is what the reference's eval_model computes with its batch_size=1 loader (RektNet/train_eval.py:115-138, 258)
  distances    sqrt((sx (px - tx))^2 + (sy (py - ty))^2), the closed form of utils.calculate_distance (utils.py:239-244) on points
               multiplied by C = 3 and input_size (train_eval.py:152-157): sx = 3 input_size[0], sy = 3 input_size[1]
  rows         both, laid out as the kernel's rows [B, 12]: loc, geo, total, d0..d6, 0, 0

Like head_refs, every function takes a torch dtype and evaluates ONE torch-CPU expression in it: float64 is the reference, float32 gives
e32 for head_refs.bound.  tests/test_kpt_eval_refs.py pins this module to outputs the reference project itself produced
(tests/golden/kpt_eval.npz)."""
import torch

import head_refs as hr

ROW = 12
GAMMA = (0.05, 0.07)
DIST_SCALE = (240.0, 240.0)          # C = 3 times input_size (80, 80)


def per_sample(hm, pts, thm, tpts, loss_type, geo, gamma_h, gamma_v, dtype):
    """-> [B, 3] float64 tensor of (location, geo, total) computed in `dtype`, sample by sample; hm / thm may be None unless l2_heatmap"""
    out = []
    for i in range(pts.shape[0]):
        s = slice(i, i + 1)
        h, t = (hm[s], thm[s]) if loss_type == "l2_heatmap" else (None, None)
        out.append(hr.cross_ratio(h, pts[s], t, tpts[s], loss_type, geo, gamma_h, gamma_v, None, dtype, want_grad=False)[0])
    return torch.stack(out)


def distances(pts, tpts, sx, sy, dtype):
    """-> [B, 7] float64 tensor of the pixel distances computed in `dtype`"""
    p, t = pts.to(dtype), tpts.to(dtype)
    dx, dy = sx * (p[..., 0] - t[..., 0]), sy * (p[..., 1] - t[..., 1])
    return torch.sqrt(dx * dx + dy * dy).double()


def rows(hm, pts, thm, tpts, loss_type, geo, gamma_h, gamma_v, sx, sy, dtype):
    """-> [B, 12] float64 tensor, the kernel's row layout"""
    B = pts.shape[0]
    out = torch.zeros(B, ROW, dtype=torch.float64)
    out[:, 0:3] = per_sample(hm, pts, thm, tpts, loss_type, geo, gamma_h, gamma_v, dtype)
    out[:, 3:10] = distances(pts, tpts, sx, sy, dtype)
    return out
