"""The reference's per-sample augmentation: parameters, random draws, and the descriptors and tables the kernels read.

* augmentation (`augment_hsv`, `augment_affine`, `data_aug`; datasets.py:226-242): torchvision 0.3's `ColorJitter(brightness=0.25,
  contrast=0.25, saturation=0.25, hue=0.04)` with probability 0.5, then `F.affine(angle, translate, scale, shear, BILINEAR, fillcolor=127)`
  of every sample that has boxes, between the patch crop and to_grayscale.  Both are glue over Pillow and are reproduced byte for byte:
  `ImageEnhance.Brightness / Contrast / Color` are `Image.blend` against 0 / the mean luma / the pixel's luma, `adjust_hue` is
  `convert('HSV')`, a wrapping uint8 shift of H and `convert('RGB')`, `F.affine` is `Image.transform(AFFINE, BILINEAR)` with the inverse
  matrix computed here in float64 (libm).  The hue shift is `int(hue_factor * 255)` truncated toward zero, modulo 256: what
  `np.uint8(float)` gave on x86-64 with the NumPy of torchvision 0.3's time (NumPy 2 raises OverflowError for the negative ones).
* random draws: per sample from `random.Random(f"{seed}/{epoch}/{index}")`, in the reference's order: the patch; with `augment_hsv or
  data_aug` the jitter gate `random()`, and when it is `> 0.5` the brightness, contrast, saturation (`uniform(0.75, 1.25)`) and hue
  (`uniform(-0.04, 0.04)`) factors and the `shuffle` of the four ops; with `augment_affine or data_aug` the gate `random()` (`> 0`), angle
  `uniform(-10, 10)`, tx, ty `uniform(-40, 40)`, scale `uniform(0.9, 1.1)`, shear `uniform(-3, 3)`; then the flip.  A sample without boxes
  returns before all of this, as in the reference.  With the three options off no extra draw happens.
* the imgaug options (`blur`, `noise`, `contrast`, `sharpen`; datasets.py:253-295, imgaug 0.3.0 over OpenCV 4.1): `iaa.GaussianBlur`,
  `iaa.AdditiveGaussianNoise(per_channel=0.5)`, `iaa.SigmoidContrast` and `iaa.Sharpen` on the 8-bit image behind the flip, in that
  order.  Neither library can be pinned here, so DESIGN §16.3 defines the bytes: the blur is OpenCV's 8-bit fixed-point separable filter
  with imgaug's kernel-size rule (cv2's own rounding is declared unpinned), the contrast imgaug's float32 256-entry table, the sharpen one
  correctly rounded double expression over imgaug's float32 matrix, and the noise a counter-based integer generator of the same
  distribution (imgaug draws from NumPy's global Mersenne stream, which no device reproduces: the distribution matches, not the stream).
  Kernel tables, the contrast tables and the sharpen coefficients are computed here and shipped with the descriptors.  Draws continue the
  sample's stream behind the flip in the reference's order: blur gate `random()` (`> 0.2`), `uniform(40, -40)` (drawn and discarded, as
  the reference does), sigma `uniform(0, 3)`; noise gate (`> 0.3`), scale `uniform(0, 7.65)`; contrast gate (`> 0.5`), cutoff
  `uniform(0.45, 0.75)`, gain `randint(5, 10)`; sharpen gate (`> 0.3`), alpha `uniform(0, 0.5)`.  imgaug's own draws (the per_channel coin
  and the noise seed) come from a second generator, `random.Random(f"{seed}/{epoch}/{index}/imgaug")`.  With the four options off no
  extra draw happens and no extra launch runs.
"""
import math
from functools import lru_cache

import numpy as np

AUG_DESC = 24                            # MDCV_IMGAUG_DESC
FX_DESC = 24                             # MDCV_IMGFX_DESC
FX_MAX_R = 7                             # csrc/imgfx_desc.h IMGFX_MAX_R
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3        # ColorJitter.get_params appends its four ops in this order
_F32 = np.float32


# ---------------------------------------------------------------------------------------------------- ColorJitter and affine
class Augmentation:
    """One sample's ColorJitter / affine parameters.  jitter: None or (order, (brightness, contrast, saturation), hue) with `order` the
    shuffled permutation of (BRIGHTNESS, CONTRAST, SATURATION, HUE); affine: None or (angle, (tx, ty), scale, shear).  `matrix` (the six
    doubles Image.transform gets) is filled in by `plan()`; `hue_shift` is the uint8 added to H.  The contrast op's grey level is the
    one value only the device knows: the mean luma of the patch at that point of the chain."""

    def __init__(self, jitter=None, affine=None):
        self.jitter, self.affine, self.matrix, self.hue_shift = None, None, None, 0
        if jitter is not None:
            order, factors, hue = jitter
            if sorted(order) != [0, 1, 2, 3] or len(factors) != 3:
                raise ValueError(f"jitter {jitter!r}: the order must be a permutation of 0..3, with three factors and a hue")
            self.jitter = (tuple(int(o) for o in order), tuple(float(f) for f in factors), float(hue))
            self.hue_shift = hue_shift(self.jitter[2])
        if affine is not None:
            angle, (tx, ty), scale, shear = affine
            self.affine = (float(angle), (float(tx), float(ty)), float(scale), float(shear))

    def __bool__(self):
        return self.jitter is not None or self.affine is not None


def hue_shift(hue_factor):
    """adjust_hue's `np.uint8(hue_factor * 255)`: truncated toward zero, modulo 256"""
    return int(hue_factor * 255) % 256


def draw_augmentation(rng, jitter_on, affine_on):
    """The draws of datasets.py:226-242 from `rng`, in its order (ColorJitter.get_params draws the four factors, then shuffles the ops)."""
    jitter = affine = None
    if jitter_on and rng.random() > 0.5:
        factors = tuple(rng.uniform(0.75, 1.25) for _ in range(3))
        hue = rng.uniform(-0.04, 0.04)
        order = [BRIGHTNESS, CONTRAST, SATURATION, HUE]
        rng.shuffle(order)
        jitter = (tuple(order), factors, hue)
    if affine_on and rng.random() > 0:
        angle = rng.uniform(-10, 10)
        translate = (rng.uniform(-40, 40), rng.uniform(-40, 40))
        scale = rng.uniform(0.9, 1.1)
        shear = rng.uniform(-3, 3)
        affine = (angle, translate, scale, shear)
    return Augmentation(jitter, affine)


def inverse_affine_matrix(width, height, angle, translate, scale, shear):
    """torchvision 0.3 F.affine's data for Image.transform(AFFINE): output pixel centre -> input position, about the centre
    (W / 2 + 0.5, H / 2 + 0.5).  float64 with libm, the form fixed: the device reproduces Pillow only from the same six doubles."""
    cx, cy = width * 0.5 + 0.5, height * 0.5 + 0.5
    a, sh = math.radians(angle), math.radians(shear)
    k = 1.0 / scale
    d = math.cos(a + sh) * math.cos(a) + math.sin(a + sh) * math.sin(a)
    m = [math.cos(a + sh), math.sin(a + sh), 0, -math.sin(a), math.cos(a), 0]
    m = [k / d * v for v in m]
    m[2] += m[0] * (-cx - translate[0]) + m[1] * (-cy - translate[1])
    m[5] += m[3] * (-cx - translate[0]) + m[4] * (-cy - translate[1])
    m[2] += cx
    m[5] += cy
    return m


def aug_descriptor(aug):
    """MDCV_IMGAUG_DESC ints for one image (include/mdcv_hip.h); `aug` None or empty: the identity, which the kernel copies through"""
    d = np.zeros(AUG_DESC, np.int32)
    matrix, order, factors, shift = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], (0, 1, 2, 3), (1.0, 1.0, 1.0), 0
    if aug is not None and aug.jitter is not None:
        order, factors, shift = aug.jitter[0], aug.jitter[1], aug.hue_shift
        d[12] = 1
    if aug is not None and aug.affine is not None:
        if aug.matrix is None:
            raise ValueError("an affine augmentation needs its matrix (inverse_affine_matrix) before it is packed")
        matrix = aug.matrix
        d[21] = 1
    d[0:12] = np.array(matrix, np.float64).view(np.int32)
    d[13:17] = order
    d[17:20] = np.array(factors, _F32).view(np.int32)           # Image.blend takes its alpha as a C float
    d[20] = shift
    return d


# ----------------------------------------------------------------------------------------- blur / noise / contrast / sharpen
class ImageFx:
    """One sample's imgaug parameters, each None when its op does not run.  blur: sigma; noise: (scale, per_channel, seed) with seed the
    32 bits that key the device's counter-based generator; contrast: (gain, cutoff); sharpen: alpha."""

    def __init__(self, blur=None, noise=None, contrast=None, sharpen=None):
        self.blur = None if blur is None else float(blur)
        self.noise = None if noise is None else (float(noise[0]), bool(noise[1]), int(noise[2]) & 0xffffffff)
        self.contrast = None if contrast is None else (int(contrast[0]), float(contrast[1]))
        self.sharpen = None if sharpen is None else float(sharpen)
        if self.blur is not None and not (self.blur < 5.0 and blur_radius(self.blur) <= FX_MAX_R):
            raise ValueError(f"blur sigma {self.blur}: sigma must stay below 5 (kernel radius {FX_MAX_R} at most; the reference draws it below 3)")
        if self.noise is not None and not 0.0 <= self.noise[0] <= 255.0:
            raise ValueError(f"noise scale {self.noise[0]} outside [0, 255]")
        if self.sharpen is not None and not 0.0 <= self.sharpen <= 1.0:
            raise ValueError(f"sharpen alpha {self.sharpen} outside [0, 1]")

    def __bool__(self):
        return any(v is not None for v in (self.blur, self.noise, self.contrast, self.sharpen))

    def runs(self):
        """some op changes bytes: a blur whose sigma imgaug skips does not"""
        return (self.blur is not None and blur_radius(self.blur) > 0) or any(v is not None for v in (self.noise, self.contrast, self.sharpen))


def draw_imgfx(rng, second, blur_on, noise_on, contrast_on, sharpen_on):
    """The draws of datasets.py:253-295 from `rng`, in its order, unused ones included; `second()` -> the generator of imgaug's own
    draws (the per_channel coin, then the noise seed), asked for only when the noise runs."""
    blur = noise = contrast = sharpen = None
    if blur_on and rng.random() > 0.2:
        rng.uniform(40, -40)                                     # the reference's unused `angle`
        blur = rng.uniform(0, 3.00)
    if noise_on and rng.random() > 0.3:
        scale = rng.uniform(0, 0.03 * 255)
        r2 = second()
        per_channel = r2.random() < 0.5                          # per_channel=0.5: a fair coin per image
        noise = (scale, per_channel, r2.getrandbits(32))
    if contrast_on and rng.random() > 0.5:
        cutoff = rng.uniform(0.45, 0.75)
        contrast = (rng.randint(5, 10), cutoff)
    if sharpen_on and rng.random() > 0.3:
        sharpen = rng.uniform(0, 0.5)
    return ImageFx(blur, noise, contrast, sharpen)


def blur_radius(sigma):
    """imgaug 0.3.0 blur_gaussian_ (cv2 backend): 0 when the op is skipped, else the radius of its kernel size"""
    if sigma <= 1e-3:
        return 0
    k = 3.3 * sigma if sigma < 3.0 else (2.9 * sigma if sigma < 5.0 else 2.6 * sigma)
    k = int(max(k, 5))
    return (k + 1 if k % 2 == 0 else k) // 2


@lru_cache(maxsize=512)
def blur_table(sigma):
    """-> (r, half table q[0..r], centre first): the Gaussian in float64 normalised to sum 1, each tap floor(w * 256 + 0.5), the centre
    corrected so that the whole kernel sums to 256 (OpenCV 4.1's 8-bit fixed point)"""
    r = blur_radius(sigma)
    w = [math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(r + 1)]
    total = w[0] + 2.0 * sum(w[1:])
    q = [int(math.floor(v / total * 256.0 + 0.5)) for v in w]
    q[0] = 256 - 2 * sum(q[1:])
    return r, tuple(q)


@lru_cache(maxsize=64)
def sigmoid_table(gain, cutoff):
    """imgaug 0.3.0 adjust_contrast_sigmoid's uint8 table, in its float32 arithmetic; the cast truncates"""
    v = np.linspace(0, 1, 256, dtype=_F32)
    table = 0 + 255 * 1 / (1 + np.exp(_F32(gain) * (_F32(cutoff) - v)))
    return np.clip(table, 0, 255).astype(np.uint8)


def sharpen_coefficients(alpha):
    """imgaug 0.3.0 Sharpen's matrix at lightness 1: float32 arrays combined with the Python-float alpha -> (centre, neighbour) float32"""
    nochange = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=_F32)
    effect = np.array([[-1, -1, -1], [-1, 8 + 1, -1], [-1, -1, -1]], dtype=_F32)
    m = (1 - alpha) * nochange + alpha * effect
    assert m.dtype == _F32
    return m[1, 1], m[0, 0]


def fx_descriptor(fx, lut_index=0):
    """MDCV_IMGFX_DESC ints for one image (include/mdcv_hip.h); `fx` None or empty, or an op that is off: the identity"""
    d = np.zeros(FX_DESC, np.int32)
    r, q, scale, kc, kn = 1, (256, 0), 0.0, _F32(1), _F32(0)
    if fx is not None and fx.blur is not None and blur_radius(fx.blur) > 0:
        r, q = blur_table(fx.blur)
        d[0] = 1
    if fx is not None and fx.noise is not None:
        scale = fx.noise[0]
        d[10], d[11] = 1, int(fx.noise[1])
        d[12:13] = np.array([fx.noise[2]], np.uint32).view(np.int32)
    if fx is not None and fx.contrast is not None:
        d[15], d[16] = 1, lut_index
    if fx is not None and fx.sharpen is not None:
        kc, kn = sharpen_coefficients(fx.sharpen)
        d[17] = 1
    d[1] = r
    d[2:2 + len(q)] = q
    d[13:15] = np.array([scale], np.float64).view(np.int32)
    d[18:20] = np.array([kc, kn], _F32).view(np.int32)
    return d
