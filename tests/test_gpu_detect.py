"""Batched detection with the boxes drawn on the device: mdcv_detect_draw_boxes (csrc/detect_draw.hip) through the C ABI against the NumPy
oracle (tests/helpers/detect_draw_numpy.py, itself pinned against Pillow by tests/test_detect_host.py), and mdcv.yolo.detect end to end
against the same chain assembled from the existing public pieces."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import detect_cases as C  # noqa: E402
import detect_draw_numpy as D  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(ROOT, "tests", "golden")
GUARD = 0x5A
NAN_BITS = np.array([np.nan]).view(np.int64)[0]


def _bits(ratio):
    return np.array([ratio], np.float64).view(np.int64)[0]


def _layout(sizes, gap=48):
    """pool offsets with `gap` guard bytes in front of, between and behind the frames (16-byte aligned starts, as the detector packs them)"""
    offs, at = [], gap
    for w, h in sizes:
        at = (at + 15) // 16 * 16
        offs.append(at)
        at += 3 * w * h + gap
    return offs, at


def _run(desc, boxes, count, pool, K, colour=(255, 0, 0)):
    """one mdcv_detect_draw_boxes call -> (pool, frame_boxes, rects, skipped) as NumPy; the tables start as the oracle's fill values"""
    from mdcv import _lib
    L = _lib.lib()
    B = len(desc)
    desc = np.ascontiguousarray(desc, np.int64).reshape(B, 6)
    d_desc = torch.from_numpy(desc.copy()).cuda()
    d_boxes = torch.from_numpy(np.ascontiguousarray(boxes, np.float32)).cuda()
    d_count = torch.from_numpy(np.ascontiguousarray(count, np.int32)).cuda()
    d_pool = torch.from_numpy(pool.copy()).cuda()
    fb = torch.full((B, K, 4), float("nan"), dtype=torch.float64, device="cuda")
    rects = torch.full((B, K, 4), -7, dtype=torch.int32, device="cuda")
    skipped = torch.full((max(B, 1),), 12345, dtype=torch.int32, device="cuda")
    rc = L.detect_draw_boxes(desc.ctypes.data, d_desc.data_ptr(), B, d_boxes.data_ptr(), d_count.data_ptr(), K, d_pool.data_ptr(), d_pool.numel(),
                             *colour, fb.data_ptr(), rects.data_ptr(), skipped.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, d_pool.cpu().numpy(), fb.cpu().numpy(), rects.cpu().numpy(), skipped.cpu().numpy()[:B]


def _check(desc, boxes, count, pool, K, colour=(255, 0, 0)):
    rc, got_pool, fb, rects, skipped = _run(desc, boxes, count, pool, K, colour)
    assert rc == 0
    want_pool, want_fb, want_rects, want_skipped = D.draw_batch(pool, desc, boxes, count, colour)
    assert np.array_equal(fb.view(np.int64), want_fb.view(np.int64))              # the doubles as bits; NaN past count[b]: not written
    assert np.array_equal(rects, want_rects)
    assert np.array_equal(skipped, want_skipped)
    assert np.array_equal(got_pool, want_pool)                                    # frames AND the guard bytes around them
    return got_pool, rects, skipped


def _golden_cases():
    z = np.load(os.path.join(G, "detect", "cases.npz"))
    names = [str(n) for n in z["names"]]
    frames = [z["frame::" + str(z[f"frame_{i}"])] for i in range(len(names))]
    K = 8
    offs, total = _layout([(f.shape[1], f.shape[0]) for f in frames])
    pool = np.full(total, GUARD, np.uint8)
    desc = np.zeros((len(names), 6), np.int64)
    boxes = np.zeros((len(names), K, 4), np.float32)
    count = np.zeros(len(names), np.int32)
    for i, f in enumerate(frames):
        pool[offs[i]:offs[i] + f.size] = f.reshape(-1)
        b = z[f"boxes_{i}"]
        boxes[i, :len(b)], count[i] = b, len(b)
        desc[i] = [offs[i], f.shape[1], f.shape[0], _bits(float(z[f"ratio_{i}"])), int(z[f"pads_{i}"][0]), int(z[f"pads_{i}"][1])]
    got, _, skipped = _check(desc, boxes, count, pool, K)
    assert not skipped.any()
    for i, f in enumerate(frames):                                                # and directly against what Pillow drew
        assert np.array_equal(got[offs[i]:offs[i] + f.size].reshape(f.shape), z[f"expected_{i}"]), names[i]


def _mixed_batch(side, transposed):
    sizes = [(1, 1), (12, 10), (37, 23), (128, 96), (301, 173)]
    if transposed:                                                                # tall frames: the pad moves to the other axis
        sizes = [(h, w) for w, h in sizes]
    K, count = 8, np.array([0, 1, 8, 3, 8], np.int32)
    rng = np.random.default_rng(side + transposed)
    offs, total = _layout(sizes)
    pool = np.full(total, GUARD, np.uint8)
    desc = np.zeros((5, 6), np.int64)
    boxes = np.zeros((5, K, 4), np.float32)
    for b, (w, h) in enumerate(sizes):
        f = C.random_frame(w, h, 50 + b)
        pool[offs[b]:offs[b] + f.size] = f.reshape(-1)
        ratio, pw, ph = C.letterbox(w, h, side)
        desc[b] = [offs[b], w, h, _bits(ratio), pw, ph]
        fb = C.frame_boxes(w, h, 300 + 10 * b + side)
        boxes[b] = C.to_detector(fb[rng.choice(len(fb), K, replace=False)], ratio, pw, ph)      # slots past count[b] hold boxes too: not drawn
        if b == 2:                                                                # every box of this frame overlaps every other
            o = np.array([[rng.uniform(-2, w / 3), rng.uniform(-2, h / 3), rng.uniform(w / 2, w + 2), rng.uniform(h / 2, h + 2)] for _ in range(K)])
            boxes[b] = C.to_detector(o, ratio, pw, ph)
        if b == 4:                                                                # boxes that must be skipped among good ones
            boxes[b, [1, 4, 6]] = C.bad_boxes()[[0, 2, 6]]
            boxes[b, 0] = C.to_detector(np.array([[3.5, 2.5, w - 4.25, h - 3.75]]), ratio, pw, ph)[0]
    assert (desc[:, 4] > 0).any() if transposed else (desc[:, 5] > 0).any()
    got, rects, skipped = _check(desc, boxes, count, pool, K)
    assert list(skipped) == [0, 0, 0, 0, 3]
    assert (got != pool).any()
    _check(desc, boxes, count, pool, K, colour=(1, 128, 254))                     # another ink: the three dword patterns of a run are distinct


def test_draw_parity():
    """the committed Pillow cases in one launch (B = 126, K = 8), then the seeded mixed batch (B = 5, K = 8, counts 0 / 1 / 8 / 3 / 8) with
    letterbox() at 64 x 64 and at 416 x 416, sizes as listed (wide frames: pad_h) and transposed (tall frames: pad_w)"""
    _golden_cases()
    for side in (64, 416):
        for transposed in (False, True):
            _mixed_batch(side, transposed)


def test_empty_shapes_write_nothing():
    sizes = [(12, 10), (37, 23)]
    offs, total = _layout(sizes)
    pool = np.full(total, GUARD, np.uint8)
    desc = np.array([[offs[b], w, h, _bits(1.0), 0, 0] for b, (w, h) in enumerate(sizes)], np.int64)
    boxes = np.tile(np.array([1, 1, 5, 5], np.float32), (2, 8, 1))
    for B, K, cnt in ((2, 0, [8, 8]), (0, 8, []), (2, 8, [0, 0])):
        rc, got, fb, rects, skipped = _run(desc[:B], boxes[:B, :K], np.array(cnt, np.int32), pool, K)
        assert rc == 0
        assert np.array_equal(got, pool)
        assert (fb.view(np.int64) == NAN_BITS).all() and (rects == -7).all()
        if K == 0 or B == 0:
            assert (skipped == 12345).all()                                       # nothing enqueued, not even the counter's memset
        else:
            assert not skipped.any()


# ------------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def mini():
    from mdcv.yolo.models import Darknet
    cwd = os.getcwd()
    os.chdir(os.path.join(G, "mini"))
    try:
        net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32")
        net.load_weights("mini.weights", net.get_start_weight_dim())
    finally:
        os.chdir(cwd)
    return net.cuda().eval()


@pytest.fixture(scope="module")
def frames():
    z = np.load(os.path.join(G, "imgload", "frames.npz"))
    fr = [np.ascontiguousarray(z[k]) for k in sorted(z.files)]
    assert len(fr) == 4 and len({f.shape for f in fr}) > 1                        # a mixed-size batch
    return fr


def _reference(net, frames, conf, nms, groups, max_boxes=200):
    """the chain from the existing public pieces, one call of each per batch of `groups`: transform_batch (pad mode) -> model ->
    detect_postprocess -> Python doubles on the host -> the NumPy oracle"""
    from mdcv.data import images as I
    from mdcv.yolo.postprocess import detect_postprocess
    W, H = net.img_size()
    out, at, outputs = [], 0, []
    for n in groups:
        fr = frames[at:at + n]
        at += n
        geoms = [I.sample_geometry(f.shape[1], f.shape[0], W, H, ts=False) for f in fr]
        with torch.no_grad():
            pred = net(I.transform_batch(fr, geoms, bw=net.get_bw()))
            outputs.append(pred)
            det = detect_postprocess(pred, None, conf, nms, 0.5, W, H, 200) if conf is not None else None
        if det is None:
            continue
        for b, (f, g) in enumerate(zip(fr, geoms)):
            d = det.image(b)
            k = min(len(d["boxes"]), max_boxes)
            ann, fb, rects, skipped = D.draw_boxes(f, d["boxes"][:k].cpu().numpy(), g.ratio, g.pad_w, g.pad_h)
            out.append(dict(boxes=fb, prob=d["prob"][:k].cpu().numpy(), rects=rects, skipped=skipped, annotated=ann))
    return out, outputs


@pytest.fixture(scope="module")
def conf_thres(mini, frames):
    """from the model's own objectness on these frames: between the 6th and the 7th highest of the frame where those are lowest, so
    that every frame keeps candidates"""
    _, outputs = _reference(mini, frames, None, None, [4])
    obj = outputs[0][..., 4].cpu().numpy()
    s = -np.sort(-obj, axis=1)
    return float(((s[:, 5].astype(np.float64) + s[:, 6]) / 2).min())


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.boxes.dtype == np.float64 and np.array_equal(g.boxes.view(np.int64), w["boxes"].view(np.int64))
        assert np.array_equal(g.prob, w["prob"]) and np.array_equal(g.rects, w["rects"]) and g.skipped == w["skipped"]
        ann = g.annotated.cpu().numpy() if torch.is_tensor(g.annotated) else g.annotated
        assert ann.dtype == np.uint8 and np.array_equal(ann, w["annotated"])


def test_detect_frames_end_to_end(mini, frames, conf_thres):
    from mdcv.yolo.detect import FrameDetector
    nms = mini.get_threshs()[1]
    want, _ = _reference(mini, frames, conf_thres, nms, [4])
    det = FrameDetector(mini, conf_thres=conf_thres)
    assert det.nms_thres == nms and (det.width, det.height) == (64, 64)
    got = list(det.detect_frames(frames))
    drawn = sum(int((r.rects[:, 2] >= 0).sum()) for r in got)
    print("conf_thres", conf_thres, "boxes per frame", [len(r.boxes) for r in got], "drawn", drawn)
    assert drawn >= 4 and all(len(r.boxes) <= det.max_boxes for r in got)         # not vacuous
    assert any((r.annotated != f).any() for r, f in zip(got, frames))
    for r in got:
        assert (np.diff(r.prob) <= 0).all()                                       # most confident first
    _same(got, want)
    # two batches (3 + 1): both staging slots; the same chain at that composition, and the same results as in one batch
    got3 = list(FrameDetector(mini, conf_thres=conf_thres, batch_size=3).detect_frames(iter(frames)))
    _same(got3, _reference(mini, frames, conf_thres, nms, [3, 1])[0])
    _same(got3, want)
    # the pixels stay on the device
    kept = list(det.detect_frames(frames, keep_on_device=True))
    assert all(torch.is_tensor(r.annotated) and r.annotated.is_cuda and r.annotated.shape == f.shape for r, f in zip(kept, frames))
    _same(kept, want)
    # max_boxes caps what is mapped and drawn, most confident first
    capped = list(FrameDetector(mini, conf_thres=conf_thres, max_boxes=1).detect_frames(frames))
    _same(capped, _reference(mini, frames, conf_thres, nms, [4], max_boxes=1)[0])


def test_file_round_trip(mini, frames, conf_thres, tmp_path):
    from PIL import Image
    from mdcv.yolo import detect as DT
    nms = mini.get_threshs()[1]
    src, out1, out2 = tmp_path / "in", tmp_path / "single", tmp_path / "dir"
    for d in (src, out1, out2):
        os.makedirs(d)
    names = [f"frame_{i}.png" for i in range(len(frames))]
    for n, f in zip(names, frames):
        Image.fromarray(f).save(src / n)
    (src / "notes.txt").write_text("not an image")
    one = list(DT.FrameDetector(mini, conf_thres=conf_thres, batch_size=1).detect_frames(frames))
    assert sum(len(r.boxes) for r in one) >= 4
    for n, r in zip(names, one):
        path = DT.single_img_detect(str(src / n), str(out1), "image", mini, "cuda:0", conf_thres, nms)
        assert path == os.path.join(str(out1), n)                                 # detect.py:107-108
        assert np.array_equal(np.asarray(Image.open(path)), r.annotated)
    assert DT.detect(str(src / names[0]), str(out1), mini, "cuda:0", conf_thres, nms) == os.path.join(str(out1), names[0])
    whole = list(DT.FrameDetector(mini, conf_thres=conf_thres).detect_frames(frames))
    paths = DT.detect(str(src), str(out2), mini, "cuda:0", conf_thres, nms)
    assert paths == [os.path.join(str(out2), n) for n in names]
    for p, r in zip(paths, whole):
        assert np.array_equal(np.asarray(Image.open(p)), r.annotated)
    # any other mode writes over the input file, as the reference does with its dumped video frames (detect.py:109-111)
    victim = str(src / names[1])
    assert DT.single_img_detect(victim, str(out1), "video", mini, "cuda:0", conf_thres, nms) == victim
    assert np.array_equal(np.asarray(Image.open(victim)), one[1].annotated)
