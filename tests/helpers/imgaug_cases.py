"""Readers of tests/golden/imgaug (tests/golden/make_golden_imgaug.py) shared by the host and GPU tests of the augmented loader."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
G, GL = os.path.join(GOLDEN, "imgaug"), os.path.join(GOLDEN, "imgload")
NAMES = ["f0", "f1", "f2", "f3"]


def npz(name):
    return np.load(os.path.join(G, name))


def frames():
    z = np.load(os.path.join(GL, "frames.npz"))
    return {k: z[k] for k in z.files}


def unpack_aug(v):
    """the 15 doubles of the generator's pack_aug -> (jitter or None, affine or None) in mdcv.data.images.Augmentation's form"""
    jitter = (tuple(int(o) for o in v[1:5]), tuple(float(f) for f in v[5:8]), float(v[8])) if v[0] else None
    affine = (float(v[10]), (float(v[11]), float(v[12])), float(v[13]), float(v[14])) if v[9] else None
    return jitter, affine


def cases():
    z = npz("cases.npz")
    out = []
    for i in range(int(z["n"])):
        fi, ts, patch, flip, bw, W, H = (int(v) for v in z[f"c{i}_params"])
        jitter, affine = unpack_aug(z[f"c{i}_aug"])
        out.append(dict(i=i, name=NAMES[fi], ts=bool(ts), patch=patch, flip=bool(flip), bw=bool(bw), W=W, H=H, scale=float(z[f"c{i}_scale"]),
                        jitter=jitter, affine=affine, patch_u8=z[f"c{i}_patch"], u8=z[f"c{i}_u8"], labels=z[f"c{i}_labels"],
                        changed=z[f"c{i}_changed"], empty=NAMES[fi] == "f3"))
    return out, int(z["T"])


def geometry(I, c, frs):
    """the sample's geometry with its augmentation attached (box-free samples are never augmented or flipped)"""
    f = frs[c["name"]]
    g = I.sample_geometry(f.shape[1], f.shape[0], c["W"], c["H"], c["ts"], c["scale"], c["patch"], c["flip"] and not c["empty"])
    g.aug = None
    if not c["empty"] and (c["jitter"] or c["affine"]):
        g.aug = I.Augmentation(c["jitter"], c["affine"])
        if c["affine"]:
            g.aug.matrix = I.inverse_affine_matrix(c["W"], c["H"], *c["affine"])
    return g
