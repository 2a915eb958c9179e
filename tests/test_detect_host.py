"""Host half of batched detection (mdcv/yolo/detect.py) and the NumPy oracle of csrc/detect_draw.hip (tests/helpers/detect_draw_numpy.py),
pinned against the committed Pillow results and against live ImageDraw; no GPU needed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import detect_cases as C  # noqa: E402
import detect_draw_numpy as D  # noqa: E402
from mdcv.data import images as I  # noqa: E402
from mdcv.yolo import detect as DT  # noqa: E402

G = os.path.join(ROOT, "tests", "golden", "detect")


def golden_cases():
    z = np.load(os.path.join(G, "cases.npz"))
    for i, name in enumerate(z["names"]):
        yield (str(name), z["frame::" + str(z[f"frame_{i}"])], z[f"boxes_{i}"], float(z[f"ratio_{i}"]), int(z[f"pads_{i}"][0]),
               int(z[f"pads_{i}"][1]), z[f"expected_{i}"])


def test_oracle_equals_every_golden_case():
    n = drawn = 0
    for name, frame, boxes, ratio, pw, ph, want in golden_cases():
        got, fb, rects, skipped = D.draw_boxes(frame, boxes, ratio, pw, ph)
        assert skipped == 0, name
        assert np.array_equal(got, want), name
        assert fb.dtype == np.float64 and rects.dtype == np.int32 and len(rects) == len(boxes)
        n += 1
        drawn += int((got != frame).any())
    assert n >= 100 and drawn >= n // 3                        # the fixture is not a set of untouched frames


def _python_doubles(b, ratio, pw, ph):
    return (b[0].item() / ratio - pw, b[1].item() / ratio - ph, b[2].item() / ratio - pw, b[3].item() / ratio - ph)   # detect.py:100-103


@pytest.mark.parametrize("W,H", C.SIZES)
def test_oracle_equals_live_imagedraw(W, H):
    pytest.importorskip("PIL")
    from PIL import Image, ImageDraw
    frame = C.random_frame(W, H, 5)
    seen = dict(low=0, high=0, outside=0, frac=0, deg_w=0, deg_h=0, deg_both=0, last=0, past=0)
    for si, (ratio, pw, ph) in enumerate(C.settings(W, H)):
        det = C.to_detector(C.frame_boxes(W, H, 40 + si), ratio, pw, ph)
        assert len(det) >= 200
        acc_im, acc = Image.fromarray(frame.copy()), frame.copy()
        for b in det:
            xy = _python_doubles(b, ratio, pw, ph)
            im = Image.fromarray(frame.copy())
            ImageDraw.Draw(im).rectangle(xy, outline="red")
            ImageDraw.Draw(acc_im).rectangle(xy, outline="red")
            got, fb, rects, skipped = D.draw_boxes(frame, b[None], ratio, pw, ph)
            assert skipped == 0 and tuple(fb[0]) == xy                     # the same doubles, bit for bit
            assert tuple(rects[0]) == tuple(int(v) for v in xy)
            assert np.array_equal(got, np.asarray(im)), (xy, ratio, pw, ph)
            acc = D.draw_boxes(acc, b[None], ratio, pw, ph)[0]
            x0, y0, x1, y1 = (int(v) for v in rects[0])
            seen["low"] += x0 < 0 <= x1 or y0 < 0 <= y1
            seen["high"] += x0 < W <= x1 or y0 < H <= y1
            seen["outside"] += x1 < 0 or y1 < 0 or x0 >= W or y0 >= H
            seen["frac"] += -1 < xy[0] < 0 or -1 < xy[1] < 0
            seen["deg_w"] += x0 == x1 and y0 != y1
            seen["deg_h"] += y0 == y1 and x0 != x1
            seen["deg_both"] += x0 == x1 and y0 == y1
            seen["last"] += x1 == W - 1 or y1 == H - 1
            seen["past"] += x1 == W or y1 == H
        assert np.array_equal(acc, np.asarray(acc_im))                      # and drawn one over another
    assert all(v > 0 for v in seen.values()), seen


def test_pillow_refuses_what_the_oracle_skips():
    from PIL import Image, ImageDraw
    frame = C.random_frame(12, 10, 3)
    for xy in ((5.0, 1.0, 4.5, 3.0), (1.0, 6.0, 4.0, 5.9)):
        with pytest.raises(ValueError):
            ImageDraw.Draw(Image.fromarray(frame.copy())).rectangle(xy, outline="red")


@pytest.mark.parametrize("ratio,pw,ph", [(1.0, 0, 0), (5.333333333333333, 0, 1), (0.4, 7, 0)])
def test_bad_boxes_are_skipped_counted_and_leave_the_frame_untouched(ratio, pw, ph):
    frame = C.random_frame(12, 10, 9)
    bad = C.bad_boxes()
    got, fb, rects, skipped = D.draw_boxes(frame, bad, ratio, pw, ph)
    assert skipped == len(bad) and np.array_equal(got, frame)
    assert (rects == np.array(D.SKIPPED_RECT, np.int32)).all()
    assert fb.shape == (len(bad), 4)                                        # the doubles are still reported
    good = np.array([[2, 2, 6, 5]], np.float32)
    mixed = np.concatenate([bad[:3], good, bad[3:]])
    got, _, rects, skipped = D.draw_boxes(frame, mixed, ratio, pw, ph)
    assert skipped == len(bad) and np.array_equal(got, D.draw_boxes(frame, good, ratio, pw, ph)[0])
    assert (2.0 ** 30 - 1 < D.LIMIT) and not D.box_ok([0.0, 0.0, 2.0 ** 30, 1.0]) and D.box_ok([0.0, 0.0, 2.0 ** 30 - 0.5, 1.0])


def test_truncation_is_toward_zero():
    _, fb, rects, _ = D.draw_boxes(np.zeros((4, 4, 3), np.uint8), np.array([[-0.9, -1.5, 2.9, 3.2]], np.float32), 1.0, 0, 0)
    assert tuple(rects[0]) == (0, -1, 2, 3)


def test_same_row_box_also_marks_the_row_below():
    """Pillow's quirk: y1 == y0 draws the end pixels of row y0 + 1 too"""
    got = D.draw_boxes(np.zeros((5, 8, 3), np.uint8), np.array([[1.2, 2.1, 5.7, 2.8]], np.float32), 1.0, 0, 0)[0]
    red = (got == np.array(D.RED, np.uint8)).all(axis=2)
    want = np.zeros((5, 8), bool)
    want[2, 1:6] = True
    want[3, 1] = want[3, 5] = True
    assert np.array_equal(red, want)


# ------------------------------------------------------------------------------------------------------ mdcv/yolo/detect.py, host half
def test_descriptors_and_pool_offsets_of_a_mixed_size_batch():
    sizes = [(1, 1), (12, 10), (37, 23), (10, 12), (301, 173)]
    plan = DT.BatchPlan(sizes, 64, 64, 8)
    offs, total = DT.frame_offsets(sizes)
    assert offs == plan.offsets and total == plan.pool_bytes
    end = 0
    for (w, h), off in zip(sizes, offs):
        assert off % 16 == 0 and off >= end                                 # aligned, in order, not overlapping
        end = off + 3 * w * h
    assert total % 16 == 0 and end <= total < end + 16
    assert plan.desc.shape == (5, DT.DETECT_DESC) and plan.desc.dtype == np.int64
    for b, (w, h) in enumerate(sizes):
        pad_w, pad_h, ratio = I.letterbox(w, h, 64, 64)
        assert list(plan.desc[b, :3]) == [offs[b], w, h] and list(plan.desc[b, 4:]) == [pad_w, pad_h]
        assert plan.desc[b, 3:4].view(np.float64)[0] == ratio
        assert plan.frefs[b] == (offs[b], 3 * w, plan.geoms[b].window[0], plan.geoms[b].window[1])
    assert plan.desc[1, 5] > 0 and plan.desc[3, 4] > 0                      # a wide frame pads rows, a tall one columns
    # the byte layout: every region 16-byte aligned, in order, inside the buffer
    marks = [0, plan.det_off, plan.pool_off, plan.in_bytes, plan.fb_off, plan.rect_off, plan.prob_off, plan.count_off, plan.skip_off, plan.nbytes]
    assert marks == sorted(marks) and all(m % 16 == 0 for m in marks)
    assert plan.pool_off - plan.det_off >= 5 * DT.DETECT_DESC * 8 and plan.in_bytes - plan.pool_off == total
    assert plan.rect_off - plan.fb_off == 5 * 8 * 32 and plan.prob_off - plan.rect_off == 5 * 8 * 16
    # packing puts each frame's bytes at its offset and the descriptors in front of the pool
    frames = [C.random_frame(w, h, 20 + b) for b, (w, h) in enumerate(sizes)]
    host = np.full(plan.in_bytes, 0xAB, np.uint8)
    plan.pack(host, frames)
    assert np.array_equal(host[plan.det_off:plan.det_off + plan.desc.nbytes].view(np.int64).reshape(5, -1), plan.desc)
    for f, off in zip(frames, offs):
        assert np.array_equal(host[plan.pool_off + off:plan.pool_off + off + f.size], f.reshape(-1))
    fr = host[plan.layout.fref_off:plan.layout.fref_off + 5 * I.FREF * 8].view(np.int64).reshape(5, I.FREF)
    assert [tuple(r) for r in fr] == plan.frefs


def test_entry_point_checks_its_arguments_without_a_gpu():
    from mdcv import _lib
    L = _lib.lib()
    desc = np.array([[0, 4, 4, 0, 0, 0]], np.int64)
    desc[0, 3] = np.array([1.0]).view(np.int64)[0]
    p = desc.ctypes.data
    assert L.detect_draw_boxes(None, None, 0, None, None, 8, None, 0, 255, 0, 0, None, None, None, None) == 0        # B == 0
    assert L.detect_draw_boxes(p, p, 1, None, p, 0, p, 48, 255, 0, 0, None, None, p, None) == 0                      # K == 0: nothing launched
    assert L.detect_draw_boxes(p, p, 1, None, p, 0, p, 47, 255, 0, 0, None, None, p, None) == -1                     # frame outside the pool
    assert L.detect_draw_boxes(p, p, 1, None, p, 0, p, 48, 256, 0, 0, None, None, p, None) == -1                     # not a byte
    assert L.detect_draw_boxes(p, p, 1, None, p, 4, p, 48, 255, 0, 0, None, None, p, None) == -1                     # K > 0 needs its tables
    for bad in (0.0, -1.0, np.nan, np.inf):
        desc[0, 3] = np.array([bad]).view(np.int64)[0]
        assert L.detect_draw_boxes(p, p, 1, None, p, 0, p, 48, 255, 0, 0, None, None, p, None) == -1


def test_detect_refuses_video_containers(tmp_path):
    for name in ("clip.mp4", "clip.MOV", "clip.avi"):
        with pytest.raises(ValueError, match="cv2.*detect_frames"):
            DT.detect(str(tmp_path / name), str(tmp_path), None, "cuda:0", 0.8, 0.25)


def test_detect_refuses_a_file_that_is_not_rgb(tmp_path):
    from PIL import Image
    path = str(tmp_path / "grey.png")
    Image.fromarray(np.zeros((6, 7), np.uint8)).save(path)
    with pytest.raises(ValueError, match="mode 'L'"):
        DT.detect(path, str(tmp_path), None, "cuda:0", 0.8, 0.25)
    with pytest.raises(ValueError, match="mode 'L'"):
        DT.single_img_detect(path, str(tmp_path), "image", None, "cuda:0", 0.8, 0.25)


def test_frame_detector_checks_its_arguments():
    class Model:
        def get_threshs(self): return 0.8, 0.25, 0.5
        def get_bw(self): return False
        def img_size(self): return 64, 48
    d = DT.FrameDetector(Model())
    assert (d.conf_thres, d.nms_thres, d.width, d.height, d.outline, d.batch_size) == (0.8, 0.25, 64, 48, (255, 0, 0), 16)
    assert DT.FrameDetector(Model(), conf_thres=0.1).conf_thres == 0.1
    for kw in (dict(top_k=0), dict(top_k=513), dict(max_boxes=201), dict(batch_size=0), dict(outline=(256, 0, 0)), dict(outline=(1, 2))):
        with pytest.raises(ValueError):
            DT.FrameDetector(Model(), **kw)
