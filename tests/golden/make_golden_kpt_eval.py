"""Writes tests/golden/kpt_eval.npz from a checkout of the reference project (cv-core/MIT-Driverless-CV-TrainingInfra):

    python tests/golden/make_golden_kpt_eval.py <path to the reference checkout>

Inputs: N = 6 samples, 5 x 7 heat-maps, sample 2 with two coincident predicted key points.  Recorded, for the 3 loss types x geo on / off
(gammas 0.05 / 0.07):

    per::<tag>      [6,3] fp32  the reference CrossRatioLoss on every sample alone ([i:i+1] slices)
    eval::<tag>     [3]   fp64  what the statements of eval_model (RektNet/train_eval.py:119-135) make of them: += .item(), / batch_num
    batched::<tag>  [3]   fp32  ONE call of the reference CrossRatioLoss on the six samples together (not what eval_model reports)

and, with C = 3 and input_size (80, 80) as print_kpt_L2_distance scales the points (train_eval.py:152-157):

    dist            [6,7] fp32  utils.calculate_distance per sample
    dist_mean / dist_total / dist_std   utils.calculate_mean_distance on the six lists

RektNet/utils.py cannot be imported (cv2, google.cloud, an rmtree at import): the two function definitions are taken out of its file with
`ast` at generation time and executed here.  The fixture is DATA (inputs + expected outputs); no reference source is stored."""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LOSS_TYPES = ("l2_softargmax", "l2_heatmap", "l1_softargmax")
N, H, W = 6, 5, 7


def reference_functions(path, names):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names)
    ns = {"np": np}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def main(ref):
    sys.path.insert(0, os.path.join(ref, "RektNet"))
    from cross_ratio_loss import CrossRatioLoss                                  # reference
    calculate_distance, calculate_mean_distance = reference_functions(os.path.join(ref, "RektNet", "utils.py"),
                                                                      ["calculate_distance", "calculate_mean_distance"])
    g = torch.Generator().manual_seed(1806)
    hm = torch.softmax(torch.randn(N, 7, H * W, generator=g) * 2, -1).view(N, 7, H, W)
    thm = torch.softmax(torch.randn(N, 7, H * W, generator=g) * 3, -1).view(N, 7, H, W)
    pts = torch.rand(N, 7, 2, generator=g)
    tpts = torch.rand(N, 7, 2, generator=g) * (79.0 / 80.0)
    pts[2, 3] = pts[2, 1]                                                        # coincident: d31 is the zero vector
    out = dict(hm=hm, thm=thm, pts=pts, tpts=tpts, gamma=np.array([0.05, 0.07]), input_size=np.array([80, 80]), C=3)
    for lt in LOSS_TYPES:
        for geo in (False, True):
            loss_function = CrossRatioLoss(lt, geo, 0.05, 0.07)
            per = np.zeros((N, 3), np.float32)
            loss_sums = [0, 0, 0]                                                # train_eval.py:119-131
            batch_num = 0
            with torch.no_grad():
                for i in range(N):
                    s = slice(i, i + 1)
                    loc_loss, geo_loss, loss = loss_function(hm[s], pts[s], thm[s], tpts[s])
                    per[i] = [loc_loss.item(), geo_loss.item(), loss.item()]
                    loss_sums[0] += loc_loss.item()
                    loss_sums[1] += geo_loss.item()
                    loss_sums[2] += loss.item()
                    batch_num += 1
                b = loss_function(hm, pts, thm, tpts)
            tag = f"{lt}:{int(geo)}"
            out[f"per::{tag}"] = per
            out[f"eval::{tag}"] = np.array([loss_sums[0] / batch_num, loss_sums[1] / batch_num, loss_sums[2] / batch_num], np.float64)
            out[f"batched::{tag}"] = np.array([float(b[0]), float(b[1]), float(b[2])], np.float32)
    input_size = (80, 80)
    C = 3                                                                        # x_batch.shape[1]
    kpt_distances = []
    for i in range(N):                                                           # train_eval.py:152-159, 171
        pred_points = pts[i:i + 1] * C
        pred_points = pred_points.data.cpu().numpy()
        pred_points *= input_size
        target_points = tpts[i:i + 1] * C
        target_points = target_points.data.cpu().numpy()
        target_points *= input_size
        kpt_distances.append(calculate_distance(target_points, pred_points))
    final_stats, total_dist, final_stats_std = calculate_mean_distance(kpt_distances)
    out["dist"] = np.array(kpt_distances)
    out["dist_mean"], out["dist_total"], out["dist_std"] = np.array(final_stats), np.array(total_dist), np.array(final_stats_std)
    assert out["dist"].dtype == np.float32 and out["dist_mean"].dtype == np.float32 and out["dist_std"].dtype == np.float32
    np.savez(os.path.join(HERE, "kpt_eval.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()})
    print("wrote kpt_eval.npz,", os.path.getsize(os.path.join(HERE, "kpt_eval.npz")), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
