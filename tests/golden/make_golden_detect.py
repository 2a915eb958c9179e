"""Writes tests/golden/detect/cases.npz and meta.json: what Pillow's ImageDraw makes of the tail of the reference's single_img_detect
(CVC-YOLOv3/detect.py:99-104).  Needs Pillow only:

    python tests/golden/make_golden_detect.py

Per case i: `frame_i` (index into the frames `frame::<W>x<H>`), `boxes_i` float32 [n,4] corner boxes in detector coordinates, `ratio_i`
(float64), `pads_i` (pad_w, pad_h) and `expected_i`, the frame after

    x0 = boxes[k, 0].item() / ratio - pad_w ... ; ImageDraw.Draw(im).rectangle((x0, y0, x1, y1), outline="red")

for every box in order, in Python doubles on `float32.item()` values as the reference computes them.  The boxes are the seeded categories
of tests/helpers/detect_cases.py (edges, corners, outside, (-1, 0), degenerate, exactly W - 1 / W), eight per case, under four (ratio, pads)
settings per frame size; case names ending in `overlap` draw eight boxes over one another, `empty` draws none.  Every box is one Pillow
accepts: the skipped kinds (inverted, NaN, inf, >= 2^30) have no Pillow result and are tested against the rule itself."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import detect_cases as C  # noqa: E402

GROUP, GROUPS = 8, 10


def pillow_draw(frame, boxes, ratio, pad_w, pad_h):
    from PIL import Image, ImageDraw
    im = Image.fromarray(frame.copy())
    draw = ImageDraw.Draw(im)
    for b in boxes:
        x0 = b[0].item() / ratio - pad_w
        y0 = b[1].item() / ratio - pad_h
        x1 = b[2].item() / ratio - pad_w
        y1 = b[3].item() / ratio - pad_h
        draw.rectangle((x0, y0, x1, y1), outline="red")
    return np.asarray(im, dtype=np.uint8)


def cases():
    """-> frames {name: array}, [(name, frame name, boxes, ratio, pad_w, pad_h)]"""
    frames, out = {}, []
    for si, (W, H) in enumerate(C.SIZES):
        fname = f"{W}x{H}"
        frames[fname] = C.random_frame(W, H, 100 + si)
        for ti, (ratio, pw, ph) in enumerate(C.settings(W, H)):
            det = C.to_detector(C.frame_boxes(W, H, 1000 * si + ti), ratio, pw, ph)
            step = len(det) // (GROUP * GROUPS)
            for gi in range(GROUPS):
                sel = det[gi * GROUP * step:(gi * GROUP + GROUP) * step:step]
                out.append((f"{fname}_s{ti}_g{gi}", fname, sel, ratio, pw, ph))
            if ti == 2:
                rng = np.random.default_rng(7 + si)
                fb = np.array([[rng.uniform(-2, W / 3), rng.uniform(-2, H / 3), rng.uniform(W / 2, W + 2), rng.uniform(H / 2, H + 2)]
                               for _ in range(GROUP)])
                out.append((f"{fname}_s{ti}_overlap", fname, C.to_detector(fb, ratio, pw, ph), ratio, pw, ph))
                out.append((f"{fname}_s{ti}_empty", fname, np.zeros((0, 4), np.float32), ratio, pw, ph))
    return frames, out


def main():
    import PIL
    frames, cs = cases()
    z = {f"frame::{k}": v for k, v in frames.items()}
    names = []
    for i, (name, fname, boxes, ratio, pw, ph) in enumerate(cs):
        names.append(name)
        z[f"frame_{i}"] = np.array(fname)
        z[f"boxes_{i}"] = boxes.astype(np.float32)
        z[f"ratio_{i}"] = np.float64(ratio)
        z[f"pads_{i}"] = np.array([pw, ph], np.int32)
        z[f"expected_{i}"] = pillow_draw(frames[fname], boxes, ratio, pw, ph)
    z["names"] = np.array(names)
    out = os.path.join(HERE, "detect")
    os.makedirs(out, exist_ok=True)
    np.savez_compressed(os.path.join(out, "cases.npz"), **z)
    json.dump({"pillow": PIL.__version__, "cases": len(cs), "outline": "red", "numpy": np.__version__}, open(os.path.join(out, "meta.json"), "w"),
              indent=1)
    print(len(cs), "cases,", os.path.getsize(os.path.join(out, "cases.npz")), "bytes")


if __name__ == "__main__":
    main()
