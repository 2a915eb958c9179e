"""NumPy restatement of csrc/imgfx.hip and of the host tables behind it: test infrastructure, never imported by the product.
Images are (H, W, 3) uint8; every step is integer or one correctly rounded float64 / float32 operation, so the kernel's bytes must equal
these bit for bit."""
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------------------------------ blur
def blur_ksize(sigma):
    """imgaug 0.3.0 blur_gaussian_ with the cv2 backend: None when the op is skipped, else the odd kernel size"""
    if sigma <= 1e-3:
        return None
    if sigma < 3.0:
        k = 3.3 * sigma
    elif sigma < 5.0:
        k = 2.9 * sigma
    else:
        k = 2.6 * sigma
    k = int(max(k, 5))
    return k + 1 if k % 2 == 0 else k


def gauss_weights(sigma, r):
    """the full float64 kernel, normalised to sum 1"""
    w = np.array([math.exp(-((i - r) ** 2) / (2.0 * sigma * sigma)) for i in range(2 * r + 1)], np.float64)
    return w / w.sum()


def blur_table(sigma):
    """-> (r, full int table of 2r + 1 taps): floor(w * 256 + 0.5), the centre corrected so that the taps sum to 256"""
    r = blur_ksize(sigma) // 2
    q = np.floor(gauss_weights(sigma, r) * 256.0 + 0.5).astype(np.int64)
    q[r] += 256 - q.sum()
    return r, q


def reflect101(i, n):
    i = np.abs(np.asarray(i))
    return np.where(i >= n, 2 * (n - 1) - i, i)


def blur_q(img, q):
    """separable, BORDER_REFLECT_101: t = sum q * src unrounded, then (sum q * t + 32768) >> 16"""
    r = len(q) // 2
    H, W = img.shape[:2]
    a = img.astype(np.int64)
    xs = reflect101(np.arange(-r, W + r), W)
    ys = reflect101(np.arange(-r, H + r), H)
    ax = a[:, xs]
    t = sum(int(q[k]) * ax[:, k:k + W] for k in range(2 * r + 1))
    ty = t[ys]
    v = sum(int(q[k]) * ty[k:k + H] for k in range(2 * r + 1))
    return ((v + 32768) >> 16).astype(np.uint8)


def blur(img, sigma):
    if blur_ksize(sigma) is None:
        return img.copy()
    return blur_q(img, blur_table(sigma)[1])


# ----------------------------------------------------------------------------------------------------------------------- noise
def hash32(x):
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & M32
    x ^= x >> np.uint64(16)
    return x


def noise_sum(seed, n):
    """S for sample counters n: the twelve 16-bit halves of the six hash words of (seed, n, j)"""
    n = np.asarray(n, np.uint64)
    S = np.zeros(n.shape, np.int64)
    for j in range(6):
        key = (np.uint64(seed & 0xFFFFFFFF) * np.uint64(0x9E3779B1) + np.uint64(j) * np.uint64(0x85EBCA77) + n * np.uint64(0xC2B2AE3D)) & M32
        h = hash32(hash32(key) + np.uint64(0x27D4EB2F))
        S += (h & np.uint64(0xFFFF)).astype(np.int64) + (h >> np.uint64(16)).astype(np.int64)
    return S


def noise_values(H, W, scale, per_channel, seed):
    """the int added to every (y, x, c): rint_half_even(scale * (S - 393210) / 65536), clipped to +-255"""
    at = np.arange(H * W, dtype=np.uint64).reshape(H, W, 1)
    n = at * np.uint64(3) + np.arange(3, dtype=np.uint64) if per_channel else np.repeat(at, 3, axis=2)
    z = np.float64(scale) * (noise_sum(seed, n) - 393210).astype(np.float64) / 65536.0
    return np.clip(np.rint(z), -255, 255).astype(np.int64)


def noise(img, scale, per_channel, seed):
    H, W = img.shape[:2]
    return np.clip(img.astype(np.int64) + noise_values(H, W, scale, per_channel, seed), 0, 255).astype(np.uint8)


# -------------------------------------------------------------------------------------------------------------------- contrast
def sigmoid_table(gain, cutoff):
    """imgaug 0.3.0 adjust_contrast_sigmoid for uint8, in its float32 arithmetic"""
    v = np.linspace(0, 1, 256, dtype=np.float32)
    table = 0 + 255 * 1 / (1 + np.exp(np.float32(gain) * (np.float32(cutoff) - v)))
    return np.clip(table, 0, 255).astype(np.uint8)


def contrast(img, gain, cutoff):
    return sigmoid_table(gain, cutoff)[img]


# --------------------------------------------------------------------------------------------------------------------- sharpen
def sharpen_matrix(alpha):
    """imgaug 0.3.0 Sharpen at lightness 1: float32 arrays combined with the Python-float alpha"""
    nochange = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=np.float32)
    effect = np.array([[-1, -1, -1], [-1, 8 + 1, -1], [-1, -1, -1]], dtype=np.float32)
    return (1 - alpha) * nochange + alpha * effect


def neighbours8(img):
    """(the image, the sum of its eight neighbours) as int64, BORDER_REFLECT_101"""
    H, W = img.shape[:2]
    a = img.astype(np.int64)
    p = a[reflect101(np.arange(-1, H + 1), H)][:, reflect101(np.arange(-1, W + 1), W)]
    s9 = sum(p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))
    return a, s9 - a


def sharpen_k(img, kc, kn):
    c, s8 = neighbours8(img)
    v = np.float64(np.float32(kc)) * c.astype(np.float64) + np.float64(np.float32(kn)) * s8.astype(np.float64)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def sharpen(img, alpha):
    m = sharpen_matrix(alpha)
    return sharpen_k(img, m[1, 1], m[0, 0])


# ----------------------------------------------------------------------------------------------------------------------- chain
def apply(img, blur_sigma=None, noise_args=None, contrast_args=None, sharpen_alpha=None):
    """blur (sigma), noise ((scale, per_channel, seed)), contrast ((gain, cutoff)), sharpen (alpha), in the reference's order"""
    if blur_sigma is not None:
        img = blur(img, blur_sigma)
    if noise_args is not None:
        img = noise(img, *noise_args)
    if contrast_args is not None:
        img = contrast(img, *contrast_args)
    if sharpen_alpha is not None:
        img = sharpen(img, sharpen_alpha)
    return img
