#!/usr/bin/env python3
"""Golden vectors for the real-image loader (mdcv/data/images.py, csrc/imgload.hip), written to tests/golden/imgload/.

    python tests/golden/make_golden_imgload.py <path of the reference checkout>

Expected images come from Pillow itself (its version is recorded in meta.json); expected labels from the reference's own label helpers
(CVC-YOLOv3/utils/utils.py, imported from the checkout).  The torchvision 0.3 glue that ImageLabelDataset.__getitem__ runs around them is
restated with Pillow calls: pad = a 127 canvas plus paste, resize = Image.resize(BILINEAR), hflip = FLIP_LEFT_RIGHT, to_grayscale =
convert('L'), to_tensor = uint8 / 255 in float32 (stored here as the uint8 image before the division).
The frames are synthetic "photos" (gradients, edges, noise) made from a fixed seed.  Everything stored is data.
"""
import json
import math
import os
import random
import sys
import warnings

import numpy as np
import PIL
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "imgload")

# frame sizes are uneven on purpose; f3 carries no boxes (raw-empty)
FRAME_SIZES = {"f0": (301, 173), "f1": (97, 211), "f2": (257, 129), "f3": (120, 90)}
BOXES = {   # CSV cells [x, y, h, w] (the reference's column quirk: x2 = x + col3, y2 = y + col2)
    "f0": [[20, 30, 40, 25], [150, 60, 70, 45], [260, 120, 50, 38], [5, 5, 160, 290]],
    "f1": [[10, 20, 60, 30], [50, 150, 40, 40]],
    "f2": [[30, 10, 100, 60], [200, 80, 40, 50], [120, 60, 20, 20]],
    "f3": [],
}


def make_frame(name, w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r = 255 * x / max(w - 1, 1)
    g = 255 * y / max(h - 1, 1)
    b = 128 + 100 * np.sin(x / 7.0) * np.cos(y / 11.0)
    img = np.stack([r, g, b], -1)
    img[(x // 23 + y // 17) % 2 == 0] *= 0.6                      # hard edges
    img[int(h * 0.3):int(h * 0.6), int(w * 0.4):int(w * 0.7)] = (250, 120, 10)
    img += rng.normal(0, 4, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# ---- the image chain, with Pillow
def pil_pad(img, hp, vp):
    w, h = img.size
    canvas = Image.new("RGB", (w + 2 * hp, h + 2 * vp), (127, 127, 127))
    canvas.paste(img, (hp, vp))
    return canvas


def ref_image(U, frame, ts, scale, patch_index, flip, bw, W, H, raw_empty):
    img = Image.fromarray(frame, "RGB")
    if ts:
        scaled = U.scale_image(img, scale)
        vp, hp = U.pre_tile_padding(scaled.size[0], scaled.size[1], W, H)
        padded = pil_pad(scaled, hp, vp)
        img, boundary = U.get_patch(padded, W, H, patch_index)
    else:
        vp, hp, _ = U.calculate_padding(frame.shape[0], frame.shape[1], H, W)
        img = pil_pad(img, hp, vp).resize((W, H), Image.BILINEAR)
    if not raw_empty:
        if bw:
            img = img.convert("L")
        if flip:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
    a = np.asarray(img, dtype=np.uint8)
    return a if a.ndim == 3 else a[:, :, None]


# ---- the label chain, with the reference's helpers (torch float32 tensors)
def ref_labels(U, boxes, ts, scale, frame_w, frame_h, patch_index, flip, W, H, T):
    raw = torch.tensor(boxes, dtype=torch.float)
    if len(raw) == 0:
        return torch.zeros((T, 5)).numpy()
    labels = U.add_class_dimension_to_labels(raw)
    labels = U.xyhw2xyxy_corner(labels)
    if ts:
        sw, sh = int(frame_w * scale), int(frame_h * scale)
        vp, hp = U.pre_tile_padding(sw, sh, W, H)
        class _Size:                                   # get_patch reads .size and crops; the boundary is all the labels need
            size = (sw + 2 * hp, sh + 2 * vp)

            def crop(self, box):
                return None
        _, boundary = U.get_patch(_Size(), W, H, patch_index)
        labels = U.scale_labels(labels, scale)
        labels = U.add_padding_on_each_side(labels, hp, vp)
        labels = U.filter_and_offset_labels(labels, boundary)
    else:
        vp, hp, ratio = U.calculate_padding(frame_h, frame_w, H, W)
        labels = U.add_padding_on_each_side(labels, hp, vp)
        labels = U.scale_labels(labels, ratio)
    # the rest of __getitem__, in float32 tensor arithmetic: both x columns mirrored about the patch width (no swap), corners to
    # centre / size with the reference's helper, division by the patch size, zero rows up to T
    if flip:
        labels[:, [1, 3]] = float(W) - labels[:, [1, 3]]
    labels[:, 1:5] = U.xyxy2xywh(labels[:, 1:5])
    labels[:, 1:5] = labels[:, 1:5] / torch.tensor([W, H, W, H], dtype=torch.float32)
    out = torch.zeros((T, 5), dtype=torch.float32)
    out[:len(labels)] = labels
    assert (out >= 0).all()
    return out.numpy()


def n_patches(U, fw, fh, scale, W, H):
    sw, sh = int(fw * scale), int(fh * scale)
    vp, hp = U.pre_tile_padding(sw, sh, W, H)
    return U.get_patch_spacings(sw + 2 * hp, sh + 2 * vp, W, H)[2]


def main(ref):
    sys.path.insert(0, os.path.join(ref, "CVC-YOLOv3"))
    warnings.filterwarnings("ignore")
    Image.ANTIALIAS = Image.LANCZOS                    # the name scale_image uses; Pillow 10 removed it
    from utils import utils as U
    os.makedirs(OUT, exist_ok=True)
    frames = {k: make_frame(k, w, h, i) for i, (k, (w, h)) in enumerate(FRAME_SIZES.items())}
    np.savez_compressed(os.path.join(OUT, "frames.npz"), **frames)

    # 1. plain resizes: the coefficient tables through a NumPy resampler, byte for byte
    resizes = [("f0", 150, 86, "lanczos"), ("f1", 48, 105, "lanczos"), ("f2", 64, 32, "lanczos"), ("f2", 300, 60, "lanczos"),
               ("f0", 64, 37, "bilinear"), ("f1", 96, 64, "bilinear"), ("f3", 130, 90, "bilinear"), ("f1", 97, 50, "lanczos")]
    rz = {}
    for i, (k, w, h, f) in enumerate(resizes):
        rz[f"r{i}_params"] = np.array([list(FRAME_SIZES).index(k), w, h, 0 if f == "lanczos" else 1], np.int64)
        rz[f"r{i}_out"] = np.asarray(Image.fromarray(frames[k]).resize((w, h), Image.LANCZOS if f == "lanczos" else Image.BILINEAR))
    np.savez_compressed(os.path.join(OUT, "resize.npz"), n=len(resizes), **rz)

    # 2. the whole chain per sample: (frame, ts, scale, patch, flip, bw, W, H)
    cases = []
    cases += [("f0", 1, 0.5, p, p % 2, 0, 64, 64) for p in range(n_patches(U, 301, 173, 0.5, 64, 64))]   # downscale, every patch
    cases += [("f0", 1, 0.5, p, 0, 0, 96, 64) for p in (0, 3)]
    cases += [("f2", 1, 1.0, p, 0, 0, 64, 64) for p in (0, 6, 14)]          # scale 1.0; rows at 32.5 -> 32 (banker's rounding)
    cases += [("f1", 1, 1.5, p, 1, 0, 96, 64) for p in (0, 9)]                    # upscale, last patch
    cases += [("f1", 1, 0.5, p, 0, 0, 64, 64) for p in (0, 1)]                    # padding on x
    cases += [("f1", 1, 0.25, 0, 1, 1, 64, 64), ("f2", 1, 0.25, 0, 0, 0, 96, 64)]  # padding on both axes; bw
    cases += [("f0", 1, 0.3, 0, 0, 0, 64, 64), ("f0", 1, 0.3, 3, 1, 0, 64, 64), ("f2", 1, 0.3, 1, 1, 0, 64, 64),
              ("f0", 1, 0.7, 5, 0, 0, 96, 64)]                                   # scales float32 cannot hold, on boxed frames
    cases += [("f1", 1, 1.5, 3, 1, 0, 96, 64), ("f0", 1, 0.5, 2, 1, 1, 64, 64)]   # (labels: no survivor + flip), bw + flip
    cases += [("f3", 1, 0.7, 0, 1, 1, 64, 64), ("f3", 0, 1.0, 0, 1, 0, 64, 64)]   # raw-empty: no flip, no gray
    cases += [("f0", 0, 1.0, 0, 0, 0, 64, 64), ("f1", 0, 1.0, 0, 1, 0, 96, 64), ("f2", 0, 1.0, 0, 0, 1, 64, 96),
              ("f0", 0, 1.0, 0, 1, 1, 96, 64), ("f2", 0, 1.0, 0, 1, 0, 257, 129)]  # pad-and-resize (the last: same size, a copy)
    T = max(len(v) for v in BOXES.values())
    kc = {}
    for i, (k, ts, scale, patch, flip, bw, W, H) in enumerate(cases):
        fw, fh = FRAME_SIZES[k]
        empty = len(BOXES[k]) == 0
        kc[f"c{i}_params"] = np.array([list(FRAME_SIZES).index(k), ts, patch, flip, bw, W, H], np.int64)
        kc[f"c{i}_scale"] = np.float64(scale)
        kc[f"c{i}_u8"] = ref_image(U, frames[k], ts, scale, patch, flip, bw, W, H, empty)
        kc[f"c{i}_labels"] = ref_labels(U, BOXES[k], ts, scale, fw, fh, patch, flip and not empty, W, H, T)
    np.savez_compressed(os.path.join(OUT, "cases.npz"), n=len(cases), T=T, **kc)

    # 3. a dataset in the reference's CSV format (the f4 row has a negative coordinate and is skipped)
    scales = {"f0": 0.5, "f1": 0.5, "f2": 0.25, "f3": 0.3}
    with open(os.path.join(OUT, "dataset.csv"), "w") as f:
        f.write("Name,URL,Width,Height,Scale,X0,Y0,H0,W0\n")
        f.write("header,,,,,,,,\n")
        for k, (w, h) in FRAME_SIZES.items():
            f.write(",".join([f"{k}.png", "", str(w), str(h), str(scales[k])] + ['"' + json.dumps(b) + '"' for b in BOXES[k]]) + "\n")
            if k == "f1":
                f.write(",".join(["f4.png", "", "50", "50", "1.0", '"[3, -1, 10, 10]"']) + "\n")

    # 4. loader batches over that CSV with forced draws, three epochs, both modes; shuffle off
    for ts, W, H, B in ((1, 64, 64, 4), (0, 96, 64, 3)):
        files = [k for k in FRAME_SIZES for _ in range(n_patches(U, *FRAME_SIZES[k], scales[k], W, H) if ts else 1)]
        out = {"W": W, "H": H, "B": B, "T": T, "files": np.array(files)}
        rng = random.Random(1234 + ts)
        for epoch in range(3):
            draws = [(rng.randrange(n_patches(U, *FRAME_SIZES[k], scales[k], W, H)) if ts else 0, rng.random() > 0.5) for k in files]
            out[f"e{epoch}_draws"] = np.array(draws, np.int64)
            out[f"e{epoch}_u8"] = np.stack([ref_image(U, frames[k], ts, scales[k] if ts else 1.0, p, fl, 0, W, H, not BOXES[k])
                                            for k, (p, fl) in zip(files, draws)])
            out[f"e{epoch}_targets"] = np.stack([ref_labels(U, BOXES[k], ts, scales[k], *FRAME_SIZES[k], p, fl and bool(BOXES[k]), W, H, T)
                                                 for k, (p, fl) in zip(files, draws)])
        np.savez_compressed(os.path.join(OUT, f"loader_{'ts' if ts else 'pad'}.npz"), **out)

    with open(os.path.join(OUT, "meta.json"), "w") as f:
        json.dump({"pillow": PIL.__version__, "torch": torch.__version__.split("+")[0], "frames": FRAME_SIZES}, f, indent=1)
        f.write("\n")
    print("wrote", OUT, "pillow", PIL.__version__)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
