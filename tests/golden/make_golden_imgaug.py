#!/usr/bin/env python3
"""Golden vectors for the augmented real-image loader (mdcv/data/images.py, csrc/imgaug.hip), written to tests/golden/imgaug/.

    python tests/golden/make_golden_imgaug.py <path of the reference checkout>

Expected images come from Pillow itself, expected boxes from the reference's own `affine_labels` and label helpers (imported from the
checkout; utils/datasets.py imports torchvision and imgaug at module level, which are stubbed with MagicMock: nothing of them is called).
The torchvision 0.3 glue that ImageLabelDataset.__getitem__ runs for `data_aug` is restated as the Pillow calls it makes:
  ColorJitter           its four ops in the shuffled order:
    adjust_brightness     ImageEnhance.Brightness(img).enhance(f)
    adjust_contrast       ImageEnhance.Contrast(img).enhance(f)
    adjust_saturation     ImageEnhance.Color(img).enhance(f)
    adjust_hue            h, s, v = img.convert('HSV').split(); h += uint8(hue * 255) with wrap-around; merge; convert('RGB')
                          (the uint8 is int(hue * 255) truncated toward zero, modulo 256: np.uint8(float) on x86-64 before NumPy 2)
  F.affine              img.transform(img.size, AFFINE, inverse matrix about (W/2 + 0.5, H/2 + 0.5), BILINEAR, fillcolor=(127, 127, 127))
then to_grayscale = convert('L'), hflip = FLIP_LEFT_RIGHT, to_tensor = uint8 / 255 (stored as the uint8 image before the division).
Frames, boxes and the CSV are those of tests/golden/imgload (make_golden_imgload.py, imported from beside this file).
The loader batches are drawn the way the loader documents its draws: `random.Random(f"{seed}/{epoch}/{index}")`, patch, jitter, affine, flip.
Every fixture box is asserted to lie at least 0.01 px from each decision in affine_labels, so a rounding difference cannot flip a row.
Everything stored is data.
"""
import json
import math
import os
import random
import sys
import warnings
from unittest import mock

import numpy as np
import PIL
import torch
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "imgaug")
sys.path.insert(0, HERE)
import make_golden_imgload as base  # noqa: E402

SEED = 7
MARGIN = 0.01


def pil_jitter(img, order, factors, hue):
    for op in order:
        if op == 0:
            img = ImageEnhance.Brightness(img).enhance(factors[0])
        elif op == 1:
            img = ImageEnhance.Contrast(img).enhance(factors[1])
        elif op == 2:
            img = ImageEnhance.Color(img).enhance(factors[2])
        else:
            h, s, v = img.convert("HSV").split()
            a = np.array(h, dtype=np.uint8)
            a = (a.astype(np.int64) + int(hue * 255) % 256).astype(np.uint8)           # uint8 wrap-around
            img = Image.merge("HSV", (Image.fromarray(a, "L"), s, v)).convert("RGB")
    return img


def inverse_matrix(center, angle, translate, scale, shear):
    angle, shear = math.radians(angle), math.radians(shear)
    scale = 1.0 / scale
    d = math.cos(angle + shear) * math.cos(angle) + math.sin(angle + shear) * math.sin(angle)
    m = [math.cos(angle + shear), math.sin(angle + shear), 0, -math.sin(angle), math.cos(angle), 0]
    m = [scale / d * v for v in m]
    m[2] += m[0] * (-center[0] - translate[0]) + m[1] * (-center[1] - translate[1])
    m[5] += m[3] * (-center[0] - translate[0]) + m[4] * (-center[1] - translate[1])
    m[2] += center[0]
    m[5] += center[1]
    return m


def pil_affine(img, angle, translate, scale, shear):
    w, h = img.size
    m = inverse_matrix((w * 0.5 + 0.5, h * 0.5 + 0.5), angle, translate, scale, shear)
    return img.transform((w, h), Image.AFFINE, m, Image.BILINEAR, fillcolor=(127, 127, 127))


def patch_image(U, frame, ts, scale, patch_index, W, H):
    img = Image.fromarray(frame, "RGB")
    if ts:
        scaled = U.scale_image(img, scale)
        vp, hp = U.pre_tile_padding(scaled.size[0], scaled.size[1], W, H)
        img, _ = U.get_patch(base.pil_pad(scaled, hp, vp), W, H, patch_index)
        return img
    vp, hp, _ = U.calculate_padding(frame.shape[0], frame.shape[1], H, W)
    return base.pil_pad(img, hp, vp).resize((W, H), Image.BILINEAR)


def ref_image(U, frame, ts, scale, patch_index, flip, bw, W, H, jitter, affine, raw_empty):
    img = patch_image(U, frame, ts, scale, patch_index, W, H)
    if not raw_empty:
        if jitter is not None:
            img = pil_jitter(img, *jitter)
        if affine is not None:
            img = pil_affine(img, *affine)
        if bw:
            img = img.convert("L")
        if flip:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
    a = np.asarray(img, dtype=np.uint8)
    return a if a.ndim == 3 else a[:, :, None]


def margins_ok(h, w, corners, angle, translate, scale, shear):
    """float64 restatement of affine_labels' decisions: True when every box is at least MARGIN away from each of them"""
    p = corners.astype(np.float64)
    side = max(w, h)
    al, be = scale * math.cos(math.radians(angle)), scale * math.sin(math.radians(angle))
    R = np.array([[al, be, (1 - al) * (w / 2) - be * (h / 2)], [-be, al, be * w / 2 + (1 - al) * (h / 2)], [0, 0, 1]])
    T = np.eye(3)
    T[0, 2], T[1, 2] = translate
    S = np.eye(3)
    S[0, 1], S[0, 2] = math.tan(math.radians(shear[0])), -math.tan(math.radians(shear[0])) * h / 2
    S[1, 0], S[1, 2] = math.tan(math.radians(shear[1])), -math.tan(math.radians(shear[1])) * w / 2
    M = S @ T @ R
    n = len(p)
    area0 = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    xy = np.ones((n * 4, 3))
    xy[:, :2] = p[:, [0, 1, 2, 3, 0, 3, 2, 1]].reshape(n * 4, 2)
    xy = (xy @ M.T)[:, :2].reshape(n, 8)
    x, y = xy[:, 0::2], xy[:, 1::2]
    box = np.stack([x.min(1), y.min(1), x.max(1), y.max(1)], 1)
    red = max(abs(math.sin(angle * math.pi / 180)), abs(math.cos(angle * math.pi / 180))) ** 0.5
    cx, cy = (box[:, 2] + box[:, 0]) / 2, (box[:, 3] + box[:, 1]) / 2
    ww, hh = (box[:, 2] - box[:, 0]) * red, (box[:, 3] - box[:, 1]) * red
    box = np.stack([cx - ww / 2, cy - hh / 2, cx + ww / 2, cy + hh / 2], 1)
    ok = (np.abs(box) > MARGIN).all() and (np.abs(box - side) > MARGIN).all()                 # the clamp bounds
    box = np.clip(box, 0, side)
    ww, hh = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = ww * hh / (area0 + 1e-16)
        ar = np.maximum(ww / (hh + 1e-16), hh / (ww + 1e-16))
    live = area0 > 0                                           # all-zero rows (no surviving label) fail w > 4 by 4 px
    ok = ok and (np.abs(ww - 4) > MARGIN).all() and (np.abs(hh - 4) > MARGIN).all()
    ok = ok and (np.abs(ratio[live] - 0.1) > MARGIN).all() and (np.abs(ar[live] - 10) > MARGIN).all()
    return bool(ok)


def ref_labels(U, D, boxes, ts, scale, frame_w, frame_h, patch_index, flip, W, H, T, affine):
    """__getitem__'s label half with the reference's helpers; -> (targets [T,5], rows affine_labels changed [T] bool)"""
    raw = torch.tensor(boxes, dtype=torch.float)
    changed = np.zeros(T, bool)
    if len(raw) == 0:
        return torch.zeros((T, 5)).numpy(), changed
    labels = U.xyhw2xyxy_corner(U.add_class_dimension_to_labels(raw))
    if ts:
        sw, sh = int(frame_w * scale), int(frame_h * scale)
        vp, hp = U.pre_tile_padding(sw, sh, W, H)

        class _Size:
            size = (sw + 2 * hp, sh + 2 * vp)

            def crop(self, box):
                return None
        _, boundary = U.get_patch(_Size(), W, H, patch_index)
        labels = U.filter_and_offset_labels(U.add_padding_on_each_side(U.scale_labels(labels, scale), hp, vp), boundary)
    else:
        vp, hp, ratio = U.calculate_padding(frame_h, frame_w, H, W)
        labels = U.scale_labels(U.add_padding_on_each_side(labels, hp, vp), ratio)
    if affine is not None:
        angle, translate, scale_, shear = affine
        before = labels.clone()
        assert margins_ok(H, W, before[:, 1:5].numpy(), -angle, translate, scale_, (-shear, 0)), "a fixture box sits on a decision"
        labels = D.affine_labels(H, W, labels, -angle, translate, scale_, (-shear, 0))
        changed[:len(labels)] = (labels != before).any(1).numpy()
    if flip:
        labels[:, 1] = W - labels[:, 1]
        labels[:, 3] = W - labels[:, 3]
    labels[:, 1:5] = U.xyxy2xywh(labels[:, 1:5])
    labels[:, (1, 3)] /= W
    labels[:, (2, 4)] /= H
    out = torch.zeros((T, 5), dtype=torch.float32)
    out[:len(labels)] = labels
    assert (out >= 0).all()
    return out.numpy(), changed


def pack_aug(jitter, affine):
    """-> float64 [15]: jitter on, the four ops in order, the three factors, hue, affine on, angle, tx, ty, scale, shear"""
    v = np.zeros(15, np.float64)
    if jitter is not None:
        v[0], v[1:5], v[5:8], v[8] = 1, jitter[0], jitter[1], jitter[2]
    if affine is not None:
        v[9], v[10], v[11:13], v[13], v[14] = 1, affine[0], affine[1], affine[2], affine[3]
    return v


def draw_aug(rng):
    """datasets.py:226-242 with data_aug: the jitter gate and ColorJitter.get_params, then the affine gate and its five uniforms"""
    jitter = affine = None
    if rng.random() > 0.5:
        b, c, s = rng.uniform(0.75, 1.25), rng.uniform(0.75, 1.25), rng.uniform(0.75, 1.25)
        h = rng.uniform(-0.04, 0.04)
        order = [0, 1, 2, 3]
        rng.shuffle(order)
        jitter = (tuple(order), (b, c, s), h)
    if rng.random() > 0:
        angle = rng.uniform(-10, 10)
        translate = (rng.uniform(-40, 40), rng.uniform(-40, 40))
        scale = rng.uniform(0.9, 1.1)
        shear = rng.uniform(-3, 3)
        affine = (angle, translate, scale, shear)
    return jitter, affine


def main(ref):
    sys.path.insert(0, os.path.join(ref, "CVC-YOLOv3"))
    warnings.filterwarnings("ignore")
    Image.ANTIALIAS = Image.LANCZOS
    for name in ("torchvision", "imgaug", "imgaug.augmenters"):
        sys.modules.setdefault(name, mock.MagicMock())
    from utils import utils as U
    from utils import datasets as D
    os.makedirs(OUT, exist_ok=True)
    z = np.load(os.path.join(HERE, "imgload", "frames.npz"))
    frames = {k: z[k] for k in z.files}
    BOXES, SIZES = base.BOXES, base.FRAME_SIZES
    T = max(len(v) for v in BOXES.values())

    # 1. the kernel chain per sample: (frame, ts, scale, patch, flip, bw, W, H, jitter, affine)
    J = {   # contrast first / in the middle / last; factors on both sides of 1.0 and 1.0 itself; hue shifts of both signs
        "c_first": ((1, 0, 2, 3), (1.2, 0.8, 1.1), 0.03), "c_mid": ((3, 1, 0, 2), (0.8, 1.25, 0.75), -0.035),
        "c_mid2": ((0, 2, 1, 3), (1.0, 0.9, 1.0), -0.004), "c_last": ((2, 0, 3, 1), (1.25, 1.0, 0.93), 0.04),
        "c_last2": ((3, 2, 0, 1), (0.75, 1.13, 1.21), -0.02),
    }
    A = {"a0": (7.3, (12.5, -20.25), 1.05, 2.0), "a1": (-9.1, (-33.0, 18.7), 0.92, -2.6), "a2": (3.0, (5.1, 4.2), 1.09, 0.4),
         "a3": (-1.7, (-8.8, 9.9), 0.97, 1.3)}
    cases = [("f0", 1, 0.5, 0, 0, 0, 64, 64, J["c_first"], None), ("f0", 1, 0.5, 4, 0, 0, 64, 64, J["c_mid"], None),
             ("f1", 1, 0.5, 1, 0, 0, 64, 64, J["c_last"], None), ("f2", 1, 0.25, 0, 0, 0, 64, 64, J["c_mid2"], None),
             ("f0", 1, 0.5, 2, 0, 0, 64, 64, None, A["a0"]), ("f1", 1, 0.5, 0, 0, 0, 64, 64, None, A["a1"]),
             ("f2", 1, 0.25, 0, 0, 0, 64, 64, J["c_last2"], A["a2"]), ("f0", 1, 0.5, 5, 1, 0, 64, 64, J["c_mid"], A["a3"]),
             ("f3", 1, 0.3, 0, 1, 0, 64, 64, J["c_first"], A["a0"]), ("f3", 0, 1.0, 0, 0, 0, 64, 64, None, A["a1"]),   # box-free: untouched
             ("f0", 0, 1.0, 0, 1, 0, 64, 64, J["c_last"], A["a2"]),
             ("f0", 1, 0.5, 3, 1, 1, 64, 64, J["c_first"], A["a3"]), ("f1", 1, 0.5, 0, 0, 1, 64, 64, J["c_mid2"], None),   # bw
             ("f0", 1, 0.7, 5, 1, 0, 96, 64, J["c_last2"], A["a0"]), ("f2", 0, 1.0, 0, 0, 0, 128, 96, J["c_mid"], A["a1"]),
             ("f1", 0, 1.0, 0, 1, 1, 96, 128, None, A["a3"])]
    kc = {}
    for i, (k, ts, scale, patch, flip, bw, W, H, jit, aff) in enumerate(cases):
        fw, fh = SIZES[k]
        empty = len(BOXES[k]) == 0
        kc[f"c{i}_params"] = np.array([list(SIZES).index(k), ts, patch, flip, bw, W, H], np.int64)
        kc[f"c{i}_scale"] = np.float64(scale)
        kc[f"c{i}_aug"] = pack_aug(jit, aff)
        kc[f"c{i}_patch"] = np.asarray(patch_image(U, frames[k], ts, scale, patch, W, H), dtype=np.uint8)     # before any augmentation
        kc[f"c{i}_u8"] = ref_image(U, frames[k], ts, scale, patch, flip, bw, W, H, jit, aff, empty)
        kc[f"c{i}_labels"], kc[f"c{i}_changed"] = ref_labels(U, D, BOXES[k], ts, scale, fw, fh, patch, flip and not empty, W, H, T,
                                                              None if empty else aff)
    np.savez_compressed(os.path.join(OUT, "cases.npz"), n=len(cases), T=T, **kc)

    # 2. loader batches with data_aug over tests/golden/imgload/dataset.csv: the loader's own draws, three epochs, both modes; shuffle off
    scales = {"f0": 0.5, "f1": 0.5, "f2": 0.25, "f3": 0.3}
    for ts, W, H, B in ((1, 64, 64, 4), (0, 96, 64, 3)):
        files = [k for k in SIZES for _ in range(base.n_patches(U, *SIZES[k], scales[k], W, H) if ts else 1)]
        out = {"W": W, "H": H, "B": B, "T": T, "seed": SEED, "files": np.array(files)}
        for epoch in range(3):
            draws, augs, u8, tg, ch = [], [], [], [], []
            for index, k in enumerate(files):
                rng = random.Random(f"{SEED}/{epoch}/{index}")
                patch = rng.randint(0, base.n_patches(U, *SIZES[k], scales[k], W, H) - 1) if ts else 0
                jit = aff = None
                flip = False
                if BOXES[k]:
                    jit, aff = draw_aug(rng)
                    flip = rng.random() > 0.5
                draws.append((patch, flip))
                augs.append(pack_aug(jit, aff))
                u8.append(ref_image(U, frames[k], ts, scales[k] if ts else 1.0, patch, flip, 0, W, H, jit, aff, not BOXES[k]))
                t, c = ref_labels(U, D, BOXES[k], ts, scales[k], *SIZES[k], patch, flip, W, H, T, aff)
                tg.append(t)
                ch.append(c)
            out[f"e{epoch}_draws"], out[f"e{epoch}_aug"] = np.array(draws, np.int64), np.stack(augs)
            out[f"e{epoch}_u8"], out[f"e{epoch}_targets"], out[f"e{epoch}_changed"] = np.stack(u8), np.stack(tg), np.stack(ch)
        np.savez_compressed(os.path.join(OUT, f"loader_{'ts' if ts else 'pad'}.npz"), **out)

    with open(os.path.join(OUT, "meta.json"), "w") as f:
        json.dump({"pillow": PIL.__version__, "torch": torch.__version__.split("+")[0], "numpy": np.__version__, "seed": SEED,
                   "margin_px": MARGIN}, f, indent=1)
        f.write("\n")
    print("wrote", OUT, "pillow", PIL.__version__)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
