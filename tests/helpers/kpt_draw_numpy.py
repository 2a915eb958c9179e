"""NumPy restatement of csrc/kpt_detect.hip: RektNet/detect.py:40-48 (the `_hm` picture) and RektNet/utils.py:61-66 (`vis_tensor_and_save`'s
circles) for batches, and the crop windows between the detector's rects and KeypointNet.

PARITY UNPINNED against cv2 (OpenCV is not available to this project); both rules below were derived by hand from OpenCV's sources:
  * `cv2.circle(img, c, 2, colour, -1)` with LINE_8 and shift 0 is drawing.cpp's Circle(..., fill=true), which for radius 2 paints the 13
    pixels of DISC below, clipped to the image;
  * `cv2.imwrite` of a float64 array converts with convertTo(CV_8U): saturate_cast<uchar>(cvRound(v)), round-half-even.
The centre is `int(pt[0] * w)` as the NumPy of the reference's time computed it: a float32 scalar times a Python int was a float64 product.
NumPy 2 keeps float32 there and can land one pixel lower; this project follows the float64 rule.
Pure NumPy, sequential loops in the reference's order.  Test infrastructure only: the product never imports it."""
import numpy as np

from kptload_numpy import image as resize_image

F = np.float32
LIMIT = float(1 << 30)
MAX_SIDE = 4096                          # MDCV_KPTLOAD_MAX_SIDE
COLOURS_BGR = [(0, 255, 0), (255, 0, 0), (255, 255, 0), (0, 255, 255), (255, 0, 255), (127, 255, 127), (255, 127, 127)]   # utils.py:62
COLOURS_RGB = np.array([c[::-1] for c in COLOURS_BGR], np.uint8)

# the filled circle of radius 2, rows cy - 2 .. cy + 2, columns cx - 2 .. cx + 2
DISC = np.array([[0, 0, 1, 0, 0],
                 [0, 1, 1, 1, 0],
                 [1, 1, 1, 1, 1],
                 [0, 1, 1, 1, 0],
                 [0, 0, 1, 0, 0]], bool)


def draw_disc(img, cx, cy, colour):
    """cv2.circle(img, (cx, cy), 2, colour, -1) on (H, W, 3) uint8, in place"""
    H, W = img.shape[:2]
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            x, y = cx + dx, cy + dy
            if DISC[dy + 2, dx + 2] and 0 <= x < W and 0 <= y < H:
                img[y, x] = colour


def center(pt, win):
    """one key point (float32 x, y) in window (x0, y0, w, h) -> (cx, cy), or None for a point that is not drawn"""
    x0, y0, w, h = (int(v) for v in win)
    with np.errstate(all="ignore"):
        px, py = float(np.float64(F(pt[0])) * np.float64(w)), float(np.float64(F(pt[1])) * np.float64(h))
    if not (abs(px) < LIMIT) or not (abs(py) < LIMIT):          # NaN and +-inf fail this too
        return None
    return x0 + int(px), y0 + int(py)                           # int() truncates toward zero


def draw_points(pool, desc, pts, window, owner, colours=COLOURS_RGB):
    """The whole launch on a host copy of the pool, cone after cone, key point 0 to 6.  desc [n,6] int64 (off, W, H, ...), pts [M,7,2]
    float32, window [M,4], owner [M,2] -> (pool copy, centers [M,7,2] int32, skipped [n] int32)"""
    pool = np.array(pool, dtype=np.uint8, copy=True)
    desc = np.asarray(desc, np.int64).reshape(-1, 6)
    pts = np.asarray(pts, F).reshape(-1, 7, 2)
    owner = np.asarray(owner).reshape(-1, 2)
    assert (np.diff(owner[:, 0]) >= 0).all(), "owner must be image-major"
    centers = np.full((len(pts), 7, 2), -1, np.int32)
    skipped = np.zeros(len(desc), np.int32)
    for m in range(len(pts)):
        b = int(owner[m, 0])
        off, W, H = (int(v) for v in desc[b, :3])
        x0, y0, w, h = (int(v) for v in window[m])
        inside = x0 >= 0 and y0 >= 0 and w >= 1 and h >= 1 and x0 + w <= W and y0 + h <= H
        img = pool[off:off + 3 * W * H].reshape(H, W, 3)
        for i in range(7):
            c = center(pts[m, i], window[m]) if inside else None
            if c is None:
                skipped[b] += 1
                continue
            centers[m, i] = c
            draw_disc(img, c[0], c[1], colours[i])
    return pool, centers, skipped


def mosaic(hm):
    """hm [B,7,S,S] float32 -> [B,7*S,S] uint8: detect.py:40-47's statements per channel, then cv2.imwrite's conversion of `out * 255`
    (float64): rint, saturate, NaN -> 0.  A constant map (the reference's division by zero) and a map with a NaN give zeros."""
    hm = np.asarray(hm, F)
    B, _, S, _ = hm.shape
    res = np.zeros((B, 7 * S, S), np.uint8)
    for b in range(B):
        out = np.empty(shape=(0, S))                                        # :40
        for o in hm[b]:                                                     # :41
            chan = np.array(o)                                              # :42
            cmin = chan.min()                                               # :43
            cmax = chan.max()                                               # :44
            with np.errstate(all="ignore"):
                chan -= cmin                                                # :45
                chan /= cmax - cmin                                         # :46
            if cmax == cmin or np.isnan(cmin) or np.isnan(cmax):
                chan = np.zeros_like(chan)                                  # the departure
            out = np.concatenate((out, chan), axis=0)                       # :47
        with np.errstate(all="ignore"):
            v = np.rint(out * 255)                                          # :48, float64
        res[b] = np.clip(np.where(np.isnan(v), 0, v), 0, 255).astype(np.uint8)
    return res


def clip_window(rect, W, H):
    """a rect (x0, y0, x1, y1, inclusive) clipped to a W x H frame -> (x0, y0, w, h), or None for a box without a crop"""
    x0, y0, x1, y1 = (int(v) for v in rect)
    cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
    if cx1 < cx0 or cy1 < cy0:
        return None
    w, h = cx1 - cx0 + 1, cy1 - cy0 + 1
    return None if w > MAX_SIDE or h > MAX_SIDE else (cx0, cy0, w, h)


def crop_frames(frames, rects, count, per, size):
    """frames [(H, W, 3) uint8 RGB], rects [B,K,4], count [B] -> (crops [M,3,S,S] float32, owner [M,2], window [M,4], M): image-major,
    box order kept; each crop is kptload_numpy.image of the window cut out on the host"""
    crops, owner, window = [], [], []
    K = rects.shape[1]
    for b, f in enumerate(frames):
        for k in range(max(0, min(int(count[b]), K, per))):
            win = clip_window(rects[b, k], f.shape[1], f.shape[0])
            if win is None:
                continue
            x0, y0, w, h = win
            crops.append(resize_image(f[y0:y0 + h, x0:x0 + w], size))
            owner.append((b, k))
            window.append(win)
    M = len(crops)
    return (np.stack(crops) if M else np.zeros((0, 3, size, size), F), np.array(owner, np.int32).reshape(M, 2),
            np.array(window, np.int32).reshape(M, 4), M)
