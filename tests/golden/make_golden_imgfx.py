#!/usr/bin/env python3
"""Golden draws for the loader's blur / noise / contrast / sharpen options (mdcv/data/images.py), written to tests/golden/imgfx/draws.npz.

    python tests/golden/make_golden_imgfx.py <path of the reference checkout>

Runs the reference's own `ImageLabelDataset.__getitem__` (CVC-YOLOv3/utils/datasets.py) over tests/golden/imgload's frames and CSV with
every option of the four on, and records what it draws and what it hands to imgaug.  Neither torchvision nor imgaug is needed:
  torchvision   a stub whose pad / resize / hflip are the Pillow calls torchvision 0.3 makes, whose `ColorJitter` draws what
                `ColorJitter.get_params` draws (four uniforms, then the shuffle of the ops) and returns the image, and whose `affine` returns
                the image: the pixels are not the subject here, the sequence of draws is
  imgaug        a stub whose four augmenter constructors record their keyword arguments and whose `augment_images` returns its input
  random        inside utils/datasets.py the module is replaced by a recorder over `random.Random(f"{seed}/{epoch}/{index}")`, the
                loader's documented per-sample stream, so every draw `__getitem__` makes is logged in order with its kind
Stored per configuration (ts / pad, with and without data_aug) and epoch: the draw log of every sample (kind 0 random, 1 uniform,
2 randint, 3 shuffle; padded with -1) and the recorded parameters [blur, sigma, noise, scale, contrast, gain, cutoff, sharpen, alpha]
(flag 0: the gate closed or the sample has no boxes).  Everything stored is data.
"""
import os
import random
import sys
import tempfile
import types
import warnings

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "imgfx")
sys.path.insert(0, HERE)
import make_golden_imgload as base  # noqa: E402

SEED = 7
EPOCHS = 3
RANDOM, UNIFORM, RANDINT, SHUFFLE = 0, 1, 2, 3


class Recorder:
    """stands where the `random` module stands in utils/datasets.py"""

    def __init__(self):
        self.rng, self.log = None, []

    def start(self, key):
        self.rng, self.log = random.Random(key), []

    def random(self):
        v = self.rng.random()
        self.log.append((RANDOM, v))
        return v

    def uniform(self, a, b):
        v = self.rng.uniform(a, b)
        self.log.append((UNIFORM, v))
        return v

    def randint(self, a, b):
        v = self.rng.randint(a, b)
        self.log.append((RANDINT, float(v)))
        return v

    def shuffle(self, x):
        self.rng.shuffle(x)
        self.log.append((SHUFFLE, 0.0))


REC = Recorder()
CALLS = []


class _Augmenter:
    def augment_images(self, arr):
        return arr


def _constructor(name):
    def make(**kw):
        CALLS.append((name, kw))
        return _Augmenter()
    return make


def _stub_modules():
    iaa = types.ModuleType("imgaug.augmenters")
    for name in ("GaussianBlur", "AdditiveGaussianNoise", "SigmoidContrast", "Sharpen"):
        setattr(iaa, name, _constructor(name))
    iaa.Sequential = lambda children: _Augmenter()
    imgaug = types.ModuleType("imgaug")
    imgaug.augmenters = iaa

    class ColorJitter:                                           # torchvision 0.3 ColorJitter.get_params, then the image as it came
        def __init__(self, brightness, contrast, saturation, hue):
            self.b, self.c, self.s, self.h = brightness, contrast, saturation, hue

        def __call__(self, img):
            for v in (self.b, self.c, self.s):
                REC.uniform(max(0, 1 - v), 1 + v)
            REC.uniform(-self.h, self.h)
            REC.shuffle([0, 1, 2, 3])
            return img

    F = types.ModuleType("torchvision.transforms.functional")
    F.pad = lambda img, padding, fill, padding_mode: base.pil_pad(img, padding[0], padding[1])
    F.resize = lambda img, size: img.resize((size[1], size[0]), Image.BILINEAR)
    F.hflip = lambda img: img.transpose(Image.FLIP_LEFT_RIGHT)
    F.affine = lambda img, *a, **k: img
    F.to_tensor = lambda img: torch.zeros(1)
    T = types.ModuleType("torchvision.transforms")
    T.functional, T.ColorJitter = F, ColorJitter
    tv = types.ModuleType("torchvision")
    tv.transforms = T
    tv.set_image_backend = lambda name: None
    sys.modules.update({"imgaug": imgaug, "imgaug.augmenters": iaa, "torchvision": tv, "torchvision.transforms": T,
                        "torchvision.transforms.functional": F})


def recorded_params():
    """CALLS of one __getitem__ -> the nine numbers; the constant arguments are checked here"""
    v = np.zeros(9, np.float64)
    for name, kw in CALLS:
        if name == "GaussianBlur":
            assert set(kw) == {"sigma"}
            v[0], v[1] = 1, kw["sigma"]
        elif name == "AdditiveGaussianNoise":
            assert kw["loc"] == 0 and kw["per_channel"] == 0.5 and set(kw) == {"loc", "scale", "per_channel"}
            v[2], v[3] = 1, kw["scale"]
        elif name == "SigmoidContrast":
            assert set(kw) == {"gain", "cutoff"} and isinstance(kw["gain"], int)
            v[4], v[5], v[6] = 1, kw["gain"], kw["cutoff"]
        else:
            assert name == "Sharpen" and set(kw) == {"alpha"}
            v[7], v[8] = 1, kw["alpha"]
    assert [n for n, _ in CALLS] == [n for n in ("GaussianBlur", "AdditiveGaussianNoise", "SigmoidContrast", "Sharpen")
                                     if v[{"GaussianBlur": 0, "AdditiveGaussianNoise": 2, "SigmoidContrast": 4, "Sharpen": 7}[n]]]
    return v


def main(ref):
    sys.path.insert(0, os.path.join(ref, "CVC-YOLOv3"))
    warnings.filterwarnings("ignore")
    Image.ANTIALIAS = Image.LANCZOS
    _stub_modules()
    state = random.getstate()
    from utils import datasets as D                              # seeds the global generators at import; nothing here uses them
    random.setstate(state)
    D.random = REC
    os.makedirs(OUT, exist_ok=True)
    z = np.load(os.path.join(HERE, "imgload", "frames.npz"))
    out = {"seed": SEED, "epochs": EPOCHS}
    closed_blur = 0
    with tempfile.TemporaryDirectory() as tmp:
        for k in z.files:
            Image.fromarray(z[k], "RGB").save(os.path.join(tmp, k + ".png"))
        for ts, W, H in ((1, 64, 64), (0, 96, 64)):
            for data_aug in (0, 1):
                ds = D.ImageLabelDataset(os.path.join(HERE, "imgload", "dataset.csv"), tmp, W, H, augment_affine=False, num_images=-1,
                                         augment_hsv=False, lr_flip=True, ud_flip=False, bw=False, n_cpu=0, vis_batch=0, data_aug=bool(data_aug),
                                         blur=True, salt=True, noise=True, contrast=True, sharpen=True, ts=bool(ts), debug_mode=False,
                                         upload_dataset=False)
                name = f"{'ts' if ts else 'pad'}_{'aug' if data_aug else 'plain'}"
                out[f"{name}_size"] = np.array([W, H], np.int64)
                out[f"{name}_files"] = np.array([os.path.basename(f) for f in ds.img_files])
                for epoch in range(EPOCHS):
                    logs, params = [], []
                    for index in range(len(ds)):
                        REC.start(f"{SEED}/{epoch}/{index}")
                        del CALLS[:]
                        ds[index]
                        logs.append(list(REC.log))
                        params.append(recorded_params())
                        boxed = len(ds.labels[index]) > 0
                        assert boxed or not CALLS
                        closed_blur += int(boxed and params[-1][0] == 0)
                    n = max(len(l) for l in logs)
                    kinds = np.full((len(logs), n), -1, np.int64)
                    values = np.zeros((len(logs), n), np.float64)
                    for i, l in enumerate(logs):
                        kinds[i, :len(l)] = [k for k, _ in l]
                        values[i, :len(l)] = [v for _, v in l]
                    out[f"{name}_e{epoch}_kinds"], out[f"{name}_e{epoch}_values"] = kinds, values
                    out[f"{name}_e{epoch}_params"] = np.stack(params)
    assert closed_blur > 0, "no sample with a closed blur gate: pick another seed"
    np.savez_compressed(os.path.join(OUT, "draws.npz"), **out)
    print("wrote", OUT, "samples with a closed blur gate:", closed_blur)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
