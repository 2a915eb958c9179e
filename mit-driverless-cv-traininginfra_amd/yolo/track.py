"""Tracks across frames: the SORT-style tracker of csrc/track.hip (include/mdcv_track.h).

The detectors' frames stand alone: nothing says that box 3 of frame 41 is the cone that was box 5 of frame 40.  `track_boxes` takes the
box tables where the detectors leave them -- on the device -- and gives every box the id of its track: a constant-velocity Kalman filter
per track, an optimal one-to-one assignment of tracks to boxes by IoU, track birth, confirmation and death, whole sequences in one launch
and no host read.  `FrameDetector(..., track=)` and its subclasses run it on the batch's stream on their own tables.
"""
import numpy as np
import torch

from .. import _lib

SLOTS = 256                              # MDCV_TRACK_SLOTS: tracks of a sequence and boxes of a frame at most
STATE_BYTES = 41024                      # MDCV_TRACK_STATE_BYTES
CONFIRMED, BAD_BOX, DROPPED = 1, 2, 4    # MDCV_TRACK_*: the bits of a box's flags


class TrackConfig:
    """iou_thres: the least IoU of a track's predicted box and a detection that may be matched, in (0, 1]; max_age: frames a track lives
    without a detection; min_hits: matches in a row that confirm a track (every track is confirmed in the first min_hits frames);
    max_tracks: slots of a sequence, 1..256 -- a detection that finds none is dropped and counted."""

    __slots__ = ("iou_thres", "max_age", "min_hits", "max_tracks")

    def __init__(self, iou_thres=0.3, max_age=1, min_hits=3, max_tracks=SLOTS):
        self.iou_thres, self.max_age, self.min_hits, self.max_tracks = float(iou_thres), int(max_age), int(min_hits), int(max_tracks)
        if not 0.0 < self.iou_thres <= 1.0:
            raise ValueError(f"TrackConfig: iou_thres must lie in (0, 1], got {iou_thres!r}")
        if self.max_age < 0 or self.min_hits < 0 or self.max_age != max_age or self.min_hits != min_hits:
            raise ValueError(f"TrackConfig: max_age and min_hits must be integers >= 0, got {max_age!r}, {min_hits!r}")
        if not 1 <= self.max_tracks <= SLOTS or self.max_tracks != max_tracks:
            raise ValueError(f"TrackConfig: max_tracks must be an integer in 1..{SLOTS}, got {max_tracks!r}")


def check_track(who, track, max_boxes):
    """the one rule of the `track` keyword: None / False (off), True (the defaults) or a TrackConfig -> a TrackConfig or None"""
    if track is None or track is False:
        return None
    if track is not True and not isinstance(track, TrackConfig):
        raise ValueError(f"{who}: track must be True or a TrackConfig, got {track!r}")
    if max_boxes > SLOTS:
        raise ValueError(f"{who}: track= takes at most {SLOTS} boxes a frame, got max_boxes {max_boxes}")
    return TrackConfig() if track is True else track


class TrackState:
    """The state blocks of S sequences, one uint8 device tensor [S, STATE_BYTES] (`raw`; all zero = fresh), and views of it: frames,
    next_id, dropped, longest_path, most_steps int32 [S]; live, ids, cls, time_since_update, hits, hit_streak int32 [S,256]; x float64
    [S,7,256] (cx, cy, s, r and three velocities); `boxes()`.  `flags`: the uint8 [S,F,K] flags of the last call."""

    def __init__(self, S, device):
        self.raw = torch.zeros(int(S), STATE_BYTES, dtype=torch.uint8, device=device)
        self.flags = None

    def _header(self, i):
        return self.raw[:, :64].view(torch.int32)[:, i]

    frames, next_id, dropped, longest_path, most_steps = (property(lambda self, i=i: self._header(i)) for i in range(5))

    def _slots(self, i):
        return self.raw[:, 64 + 1024 * i:64 + 1024 * (i + 1)].view(torch.int32)

    live, ids, cls, time_since_update, hits, hit_streak = (property(lambda self, i=i: self._slots(i)) for i in range(6))

    @property
    def x(self):
        return self.raw[:, 6208:6208 + 7 * 2048].view(torch.float64).view(-1, 7, SLOTS)

    def boxes(self):
        """float64 [S,256,4]: every slot's state as a box (meaningful where `live`)"""
        x = self.x
        w = (x[:, 2] * x[:, 3]).sqrt()
        h = x[:, 2] / w
        return torch.stack([x[:, 0] - w / 2, x[:, 1] - h / 2, x[:, 0] + w / 2, x[:, 1] + h / 2], -1)


def launch(cfg, state_ptr, boxes_ptr, box_strides, count_ptr, count_strides, cls_ptr, cls_strides, S, F, K, id_ptr, flags_ptr, stream):
    """mdcv_track_frames on tables where they lie (strides in elements: sequence, frame)"""
    L = _lib.track_lib()
    L.check(L.track_frames(boxes_ptr, *box_strides, count_ptr, *count_strides, cls_ptr, *cls_strides, S, F, K, cfg.iou_thres, cfg.max_age,
                           cfg.min_hits, cfg.max_tracks, state_ptr, id_ptr, flags_ptr, stream), "track_frames")


def track_boxes(boxes, count, cls=None, config=None, state=None):
    """boxes: float64 device tensor [S,F,K,4] (x0, y0, x1, y1; the first count[s,f] <= 256 of a frame are read), count int32 [S,F], cls
    int32 [S,F,K] or None (with it a track only takes boxes of its class) -> (track_id int32 [S,F,K], -1 for a box without a track;
    confirmed bool [S,F,K]; state).  Passing `state` back in continues the S sequences where the last call left them.  One launch on
    the current stream, no host read."""
    cfg = TrackConfig() if config is None else config
    if not isinstance(cfg, TrackConfig):
        raise ValueError(f"track_boxes: config must be a TrackConfig, got {config!r}")
    if boxes.dim() != 4 or boxes.shape[3] != 4 or boxes.dtype != torch.float64 or boxes.shape[2] < 1:
        raise ValueError(f"track_boxes: boxes must be float64 [S,F,K,4] with K >= 1, got {tuple(boxes.shape)} {boxes.dtype}")
    S, F, K = (int(v) for v in boxes.shape[:3])
    if count.dtype != torch.int32 or tuple(count.shape) != (S, F) or count.device != boxes.device:
        raise ValueError(f"track_boxes: count must be an int32 [S,F] tensor on the boxes' device, got {tuple(count.shape)} {count.dtype}")
    if cls is not None and (cls.dtype != torch.int32 or tuple(cls.shape) != (S, F, K) or cls.device != boxes.device):
        raise ValueError(f"track_boxes: cls must be an int32 [S,F,K] tensor on the boxes' device, got {tuple(cls.shape)} {cls.dtype}")
    if state is not None and (not isinstance(state, TrackState) or state.raw.shape[0] != S or state.raw.device != boxes.device):
        raise ValueError(f"track_boxes: state must be the TrackState of an earlier call with the same {S} sequences on the same device")
    _lib.require_gpu(boxes)
    dev = boxes.device
    boxes, count = boxes.detach().contiguous(), count.contiguous()
    cls = None if cls is None else cls.contiguous()
    with torch.cuda.device(dev):
        if state is None:
            state = TrackState(S, dev)
        track_id = torch.empty(S, F, K, dtype=torch.int32, device=dev)
        flags = torch.empty(S, F, K, dtype=torch.uint8, device=dev)
        launch(cfg, state.raw.data_ptr(), boxes.data_ptr(), (F * K * 4, K * 4), count.data_ptr(), (F, 1),
               None if cls is None else cls.data_ptr(), (F * K, K), S, F, K, track_id.data_ptr(), flags.data_ptr(),
               torch.cuda.current_stream(dev).cuda_stream)
    state.flags = flags
    return track_id, (flags & CONFIRMED) != 0, state


def synthetic_scene(frames, objects, seed=0, size=(1280, 720), miss=0.1, false_pos=2, jitter=1.5, classes=0, K=None, empty=()):
    """A seeded scene for tests and timing: `objects` boxes of 20..90 pixels that cross a `size` picture at up to 12 pixels a frame, each
    missed with probability `miss`, `false_pos` random boxes a frame, Gaussian `jitter` on every coordinate, the frames in `empty` without
    a box, every frame's boxes shuffled -> boxes float64 [frames,K,4], count int32 [frames], cls int32 [frames,K] (None without
    `classes`); K defaults to the largest count."""
    rng = np.random.default_rng([int(seed), int(frames), int(objects)])
    W, H = size
    c = rng.uniform([0, 0], [W, H], (objects, 2))
    v = rng.uniform(-12, 12, (objects, 2))
    wh = rng.uniform(20, 90, (objects, 2))
    kind = rng.integers(0, max(classes, 1), objects)
    rows = []
    for f in range(frames):
        keep = rng.random(objects) >= miss
        fp_c, fp_wh = rng.uniform([0, 0], [W, H], (false_pos, 2)), rng.uniform(20, 90, (false_pos, 2))
        cc, ww = np.vstack([(c + f * v)[keep], fp_c]), np.vstack([wh[keep], fp_wh])
        b = np.hstack([cc - ww / 2, cc + ww / 2]) + jitter * rng.standard_normal((len(cc), 4))
        k = np.concatenate([kind[keep], rng.integers(0, max(classes, 1), false_pos)])
        order = rng.permutation(len(b))
        rows.append((b[order], k[order]) if f not in empty else (b[:0], k[:0]))
    K = max(max(len(b) for b, _ in rows), 1) if K is None else int(K)
    boxes, count, cls = np.zeros((frames, K, 4)), np.zeros(frames, np.int32), np.zeros((frames, K), np.int32)
    for f, (b, k) in enumerate(rows):
        n = min(len(b), K)
        boxes[f, :n], cls[f, :n], count[f] = b[:n], k[:n], n
    return boxes, count, cls if classes else None
