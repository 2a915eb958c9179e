"""NumPy restatement of csrc/detect_draw.hip: the tail of CVC-YOLOv3/detect.py:99-104 (`single_img_detect`) for one frame.

Every kept box of `Detections.boxes` (float32 corners in detector coordinates) is
  a. mapped to frame coordinates as the reference maps it on the host: `float(v) / ratio - pad` in IEEE double;
  b. validated: Pillow's `ImageDraw.rectangle` raises for x1 < x0 or y1 < y0 (compared as doubles), and C leaves the conversion of a
     non-finite or huge double to int undefined -- such a box (any coordinate NaN, +-inf or of magnitude >= 2^30) is NOT drawn, its
     rectangle is (0, 0, -1, -1) and the frame's `skipped` count goes up by one (a documented departure);
  c. truncated toward zero (C's `(int)`): -0.9 -> 0, -1.5 -> -1;
  d. rasterised as Pillow 12.2's ImagingDrawRectangle does for width 1 without fill: rows y0 and y1 from x0 to x1 inclusive, columns x0
     and x1 over every row between y0 + 1 and y1 inclusive IN EITHER ORDER -- with y1 == y0 that is row y0 + 1, which therefore gets the
     two end pixels (Pillow's quirk, reproduced) -- all clipped to the frame.
Pure NumPy, no Pillow: tests/test_detect_host.py pins it against live `ImageDraw` and against tests/golden/detect/cases.npz.
"""
import numpy as np

LIMIT = float(1 << 30)
SKIPPED_RECT = (0, 0, -1, -1)
RED = (255, 0, 0)                       # ImageColor.getrgb("red")


def map_boxes(boxes, ratio, pad_w, pad_h):
    """float32 [n,4] detector corners -> float64 [n,4] frame coordinates: Python-double arithmetic on `float32.item()` values"""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    out = np.empty(boxes.shape, np.float64)
    pads = (pad_w, pad_h, pad_w, pad_h)
    with np.errstate(all="ignore"):
        for j in range(4):
            out[:, j] = boxes[:, j].astype(np.float64) / np.float64(ratio) - np.float64(pads[j])
    return out


def box_ok(fb):
    """the validation of one mapped box (four doubles)"""
    x0, y0, x1, y1 = (float(v) for v in fb)
    for v in (x0, y0, x1, y1):
        if not (abs(v) < LIMIT):        # NaN and +-inf fail this too
            return False
    return not (x1 < x0 or y1 < y0)


def draw_rect(frame, rect, colour=RED):
    """ImagingDrawRectangle(width 1, no fill) of the int rectangle on frame (H, W, 3) uint8, in place"""
    H, W = frame.shape[:2]
    x0, y0, x1, y1 = (int(v) for v in rect)
    cx0, cx1 = max(x0, 0), min(x1, W - 1)
    if cx0 <= cx1:
        for y in (y0, y1):
            if 0 <= y < H:
                frame[y, cx0:cx1 + 1] = colour
    lo, hi = y0 + 1, max(y1, y0 + 1)
    lo, hi = max(lo, 0), min(hi, H - 1)
    for x in (x0, x1):
        if 0 <= x < W and lo <= hi:
            frame[lo:hi + 1, x] = colour


def draw_boxes(frame, boxes, ratio, pad_w, pad_h, colour=RED):
    """-> (annotated (H,W,3) uint8 copy, frame_boxes float64 [n,4], rects int32 [n,4], skipped)"""
    out = np.array(frame, dtype=np.uint8, copy=True)
    fb = map_boxes(boxes, ratio, pad_w, pad_h)
    rects = np.empty((len(fb), 4), np.int32)
    skipped = 0
    for k in range(len(fb)):
        if not box_ok(fb[k]):
            rects[k] = SKIPPED_RECT
            skipped += 1
            continue
        rects[k] = [int(v) for v in fb[k]]          # int() truncates toward zero, as C's (int)
        draw_rect(out, rects[k], colour)
    return out, fb, rects, skipped


def draw_batch(pool, desc, boxes, count, colour=RED):
    """The whole launch on a host copy of the pool: desc [B, 6] int64 (MDCV_DETECT_DESC words: off, W, H, ratio bits, pad_w, pad_h),
    boxes float32 [B,K,4], count [B].  -> (pool copy, frame_boxes [B,K,4] with NaN past count, rects [B,K,4] with -7 past count, skipped [B])"""
    pool = np.array(pool, dtype=np.uint8, copy=True)
    desc = np.asarray(desc, np.int64).reshape(-1, 6)
    B, K = len(desc), boxes.shape[1] if len(desc) else 0
    fbs = np.full((B, K, 4), np.nan, np.float64)
    rects = np.full((B, K, 4), -7, np.int32)
    skipped = np.zeros(B, np.int32)
    for b in range(B):
        off, W, H = (int(v) for v in desc[b, :3])
        ratio = float(desc[b, 3:4].view(np.float64)[0])
        n = min(int(count[b]), K)
        view = pool[off:off + 3 * W * H].reshape(H, W, 3)
        ann, fb, rc, sk = draw_boxes(view, boxes[b, :n], ratio, int(desc[b, 4]), int(desc[b, 5]), colour)
        view[:] = ann
        fbs[b, :n], rects[b, :n], skipped[b] = fb, rc, sk
    return pool, fbs, rects, skipped
