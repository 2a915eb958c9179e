"""mdcv_track_frames (csrc/track.hip) against the restatement (tests/helpers/track_numpy.py): ids and flags exactly, the
state boxes within 16 d (d: the block filter against a 7x7 one on the CPU); one launch of F frames against F launches of one frame, bit
for bit; FrameDetector(track=) end to end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import track_numpy as TN  # noqa: E402
from test_gpu_kpt_detect import kpnet, mini, scene  # noqa: E402,F401
from test_track_host import filter_yardstick  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_against_the_restatement_and_frame_by_frame(name):
    from mdcv.yolo.track import TrackConfig, track_boxes
    boxes, count, cls, kw, trackers, want_id, want_flags = TN.case(name)
    if name in "ad":
        assert any(p >= 3 for _, _, p in trackers[0].solves)                  # an augmentation that re-assigns two or more earlier rows
    if name == "d":
        assert any(nr > n >= 64 for nr, n, _ in trackers[0].solves)           # more rows than boxes: dummy columns past a lane's first register
    cfg, (S, F, K) = TrackConfig(**kw), boxes.shape[:3]
    tid, conf, state = track_boxes(dev(boxes), dev(count), dev(cls), cfg)
    assert np.array_equal(tid.cpu().numpy(), want_id) and np.array_equal(state.flags.cpu().numpy(), want_flags)
    assert np.array_equal(conf.cpu().numpy(), (want_flags & TN.CONFIRMED) != 0)
    got_boxes, bound = state.boxes().cpu().numpy(), 16 * filter_yardstick()
    for s, t in enumerate(trackers):
        for field, mine in (("frames", t.frames), ("next_id", t.next_id), ("dropped", t.dropped), ("longest_path", t.longest), ("most_steps", t.most_steps)):
            assert int(getattr(state, field)[s]) == mine, field
        want_boxes, slots = t.boxes()
        assert np.array_equal(state.live[s].cpu().numpy() != 0, t.live) and np.array_equal(state.ids[s].cpu().numpy()[slots], t.id[slots])
        assert np.array_equal(state.hit_streak[s].cpu().numpy()[slots], t.streak[slots])
        err = np.abs(got_boxes[s, slots] - want_boxes).max() if len(slots) else 0.0
        print(f"case {name}, sequence {s}: {len(slots)} live tracks, state boxes off by {err:.3g}, bound {bound:.3g}")
        assert err <= bound
    step_state, ids, flags = None, [], []
    for f in range(F):                                                        # F launches of one frame through `state`
        i, _, step_state = track_boxes(dev(boxes[:, f:f + 1]), dev(count[:, f:f + 1]), dev(None if cls is None else cls[:, f:f + 1]), cfg, step_state)
        ids.append(i)
        flags.append(step_state.flags)
    assert torch.equal(torch.cat(ids, 1), tid) and torch.equal(torch.cat(flags, 1), state.flags) and torch.equal(step_state.raw, state.raw)


def test_bad_boxes_leave_the_good_ones_unchanged():
    from mdcv.yolo.track import track_boxes
    boxes, count, _, _, _, want_id, want_flags = TN.case("e")
    good = (want_flags[0] & TN.BAD_BOX) == 0
    packed, n = np.zeros_like(boxes), np.zeros_like(count)
    for f in range(boxes.shape[1]):
        keep = np.nonzero(good[f, :count[0, f]])[0]
        packed[0, f, :len(keep)], n[0, f] = boxes[0, f, keep], len(keep)
    tid = track_boxes(dev(packed), dev(n))[0].cpu().numpy()
    for f in range(boxes.shape[1]):
        assert np.array_equal(tid[0, f, :n[0, f]], want_id[0, f, :count[0, f]][good[f, :count[0, f]]])


@pytest.mark.parametrize("kind", ["plain", "class_aware", "tiled_per_class", "cone"])
def test_detectors_with_tracking(kind, mini, kpnet, scene, monkeypatch):      # noqa: F811
    from mdcv import _lib
    from mdcv.yolo import detect as DT
    from mdcv.yolo.track import TrackConfig, track_boxes
    frames, thres = scene
    thres = 0.01 if "class" in kind else thres                                # class scores (objectness x class) lie below the scene's objectness threshold
    make = {"plain": lambda **kw: DT.FrameDetector(mini, conf_thres=thres, batch_size=2, **kw),
            "class_aware": lambda **kw: DT.FrameDetector(mini, conf_thres=thres, batch_size=2, class_aware=True, **kw),
            "tiled_per_class": lambda **kw: DT.TiledFrameDetector(mini, 1.0, conf_thres=thres, batch_size=2, class_aware=True, tile_merge="per_class", **kw),
            "cone": lambda **kw: DT.FrameConeDetector(mini, kpnet, conf_thres=thres, batch_size=2, bucket=8, max_cones=2, **kw)}[kind]
    monkeypatch.setattr(_lib, "_track", None)
    plain = list(make().detect_frames(frames))
    assert _lib._track is None and all(r.track_id is None and r.confirmed is None for r in plain)
    cfg = TrackConfig(iou_thres=0.05, min_hits=1)
    got = list(make(track=cfg).detect_frames(frames))                           # two batches, one sequence
    assert _lib._track is not None and sum(len(r.boxes) for r in got) >= 3
    K = max(max(len(r.boxes) for r in got), 1)
    boxes, count = np.zeros((1, len(got), K, 4)), np.array([[len(r.boxes) for r in got]], np.int32)
    cls = np.zeros((1, len(got), K), np.int32) if got[0].cls is not None else None
    for f, (r, p) in enumerate(zip(got, plain)):
        boxes[0, f, :len(r.boxes)] = r.boxes
        if cls is not None:
            cls[0, f, :len(r.boxes)] = r.cls
        for field in ("boxes", "prob", "rects", "skipped", "annotated", "cls"):
            assert np.array_equal(getattr(r, field), getattr(p, field)), field
    tid, conf, _ = track_boxes(dev(boxes), dev(count), dev(cls), config=cfg)
    for f, r in enumerate(got):
        assert r.track_id.dtype == np.int32 and r.confirmed.dtype == bool
        assert np.array_equal(r.track_id, tid[0, f, :len(r.boxes)].cpu().numpy()) and np.array_equal(r.confirmed, conf[0, f, :len(r.boxes)].cpu().numpy())
