"""Writes tests/golden/detect_tiles/cases.npz and meta.json: what the reference's own greedy NMS (CVC-YOLOv3/utils/nms.py `nms`) keeps of the
concatenated, offset candidates of a frame's tiles.  Run by hand with the reference checkout as its argument (needs torch on the CPU):

    python tests/golden/make_golden_detect_tiles.py /path/to/reference

Per case i: `boxes_i` float32 [T,K,4] (tile coordinates), `prob_i` float32 [T,K], `count_i` int32 [T], `tiles_i` int32 [T,4] (frame, off_x,
off_y, 0), `args_i` float64 (B, overlap, top_k) and, per frame b, `keep_i_b` int32 [n,2]: the (tile, slot) of the kept candidates in the
order `nms` returns them.  Every case is tie-free (distinct scores), so the reference's unstable CPU sort cannot matter.  The scenes are
seeded: objects in scaled-frame coordinates, each seen (clipped to the tile, jittered by whole sixteenths of a pixel) by every tile it
reaches, among clutter boxes -- so tiles overlap, duplicates exist and the top_k cut bites in some cases.  The seam rule is not the
reference's and is not part of these vectors."""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import detect_tiles_numpy as TN  # noqa: E402

F = np.float32
# (seed, B, K, patch, tiles per axis, step, objects per frame, clutter per tile, overlap, top_k)
SCENES = [(1, 1, 8, 64, 2, 48, 6, 2, 0.5, 16), (2, 2, 12, 64, 3, 40, 14, 3, 0.45, 200), (3, 3, 16, 64, 2, 56, 20, 6, 0.5, 24),
          (4, 1, 24, 96, 3, 70, 40, 8, 0.3, 64), (5, 2, 8, 64, 2, 32, 10, 1, 0.6, 200), (6, 1, 32, 64, 4, 44, 60, 10, 0.5, 200)]


def scene(seed, B, K, patch, per_axis, step, n_obj, clutter, overlap, top_k):
    rng = np.random.default_rng(seed)
    T = B * per_axis * per_axis
    boxes, prob = np.zeros((T, K, 4), F), np.zeros((T, K), F)
    count, tiles = np.zeros(T, np.int32), np.zeros((T, 4), np.int32)
    border = int(rng.integers(0, 9))                                         # a bordered frame: negative offsets
    scores = rng.permutation(T * K * 4)[:T * K].astype(np.float64)           # distinct
    scores = (0.05 + 0.9 * scores / (T * K * 4)).astype(F)
    assert len(np.unique(scores)) == T * K
    at = 0
    for b in range(B):
        side = step * (per_axis - 1) + patch
        c = rng.uniform(0, side, (n_obj, 2))
        s = rng.uniform(6, 30, (n_obj, 2))
        objs = np.concatenate([c - s / 2, c + s / 2], axis=1) - border
        for r in range(per_axis):
            for q in range(per_axis):
                t = b * per_axis * per_axis + r * per_axis + q
                ox, oy = q * step - border, r * step - border
                tiles[t] = [b, ox, oy, 0]
                local = objs - np.array([ox, oy, ox, oy])
                seen = local[(local[:, 2] > 2) & (local[:, 3] > 2) & (local[:, 0] < patch - 2) & (local[:, 1] < patch - 2)]
                seen = np.clip(seen, 0, patch) + rng.integers(-24, 25, seen.shape) / 16.0
                extra = rng.uniform(0, patch - 12, (clutter, 2))
                extra = np.concatenate([extra, extra + rng.uniform(3, 12, (clutter, 2))], axis=1)
                cand = np.concatenate([seen, extra])[rng.permutation(len(seen) + clutter)][:K]
                n = len(cand)
                order = np.argsort(-scores[at:at + n].astype(np.float64))      # a tile's slots are in descending confidence
                boxes[t, :n], prob[t, :n], count[t] = cand.astype(F), scores[at:at + n][order], n
                at += K
    return dict(boxes=boxes, prob=prob, count=count, tiles=tiles, B=B, overlap=overlap, top_k=top_k)


def reference_keep(nms, s):
    """per frame: the (tile, slot) rows `nms` keeps of the concatenated, offset candidates"""
    import torch
    out = []
    for b in range(s["B"]):
        cand, prob, src = [], [], []
        for t in np.nonzero(s["tiles"][:, 0] == b)[0]:
            n = int(s["count"][t])
            cand.append(TN.offset_boxes(s["boxes"][t, :n], s["tiles"][t, 1], s["tiles"][t, 2]))
            prob.append(s["prob"][t, :n])
            src += [(t, k) for k in range(n)]
        cand, prob = np.concatenate(cand), np.concatenate(prob)
        keep = nms(torch.from_numpy(cand), torch.from_numpy(prob), overlap=s["overlap"], top_k=s["top_k"]).numpy()
        out.append(np.array([src[i] for i in keep], np.int32).reshape(-1, 2))
    return out


def main(ref):
    import torch
    spec = importlib.util.spec_from_file_location("ref_nms", os.path.join(ref, "CVC-YOLOv3", "utils", "nms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    z, kept, cut = {}, 0, 0
    for i, sc in enumerate(SCENES):
        s = scene(*sc)
        z[f"boxes_{i}"], z[f"prob_{i}"], z[f"count_{i}"], z[f"tiles_{i}"] = s["boxes"], s["prob"], s["count"], s["tiles"]
        z[f"args_{i}"] = np.array([s["B"], s["overlap"], s["top_k"]], np.float64)
        for b, k in enumerate(reference_keep(mod.nms, s)):
            z[f"keep_{i}_{b}"] = k
            kept += len(k)
            cut += int(s["count"][s["tiles"][:, 0] == b].sum()) > s["top_k"]
    out = os.path.join(HERE, "detect_tiles")
    os.makedirs(out, exist_ok=True)
    np.savez_compressed(os.path.join(out, "cases.npz"), **z)
    json.dump({"cases": len(SCENES), "kept": kept, "frames_cut_by_top_k": cut, "torch": torch.__version__, "numpy": np.__version__},
              open(os.path.join(out, "meta.json"), "w"), indent=1)
    print(len(SCENES), "cases,", kept, "kept,", cut, "frames cut by top_k,", os.path.getsize(os.path.join(out, "cases.npz")), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
