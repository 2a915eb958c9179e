"""The tracker's rule (include/mdcv_track.h) restated in float64 and exact integers: `Tracker` is one sequence, `assign` the
row-by-row shortest-augmenting-path assignment, `case` the cases of the GPU test.  Every float64 step
is one NumPy operation in the header's order, so the quantised gains -- and with them every id -- are the kernel's."""
import functools

import numpy as np

SLOTS, DUMMY = 256, 65535
CONFIRMED, BAD_BOX, DROPPED = 1, 2, 4
QV, RV = (1e-2, 1e-2, 1e-4), (1.0, 1.0, 10.0)


def assign(cost):
    """cost: integer [nr, n] -> (column of each row, columns >= n are the dummy ones; the longest augmenting path; scan steps)"""
    cost = np.asarray(cost, np.int64)
    nr, n = cost.shape
    m = max(n, nr)
    full = np.full((nr, m), DUMMY, np.int64)
    full[:, :n] = cost
    u, v, p = np.zeros(nr, np.int64), np.zeros(m, np.int64), np.full(m, -1)
    longest = steps = 0
    for r in range(nr):
        minv, way, used, j0 = np.full(m, np.iinfo(np.int64).max), np.full(m, -1), np.zeros(m, bool), -1
        while True:
            steps += 1
            if j0 >= 0:
                used[j0] = True
            i0 = r if j0 < 0 else p[j0]
            cur = full[i0] - u[i0] - v
            lower = ~used & (cur < minv)
            minv[lower], way[lower] = cur[lower], j0
            free = np.nonzero(~used)[0]
            j1 = free[np.argmin(minv[free])]                                  # argmin: the first, i.e. lowest, column among equal minima
            delta = minv[j1]
            u[p[used]] += delta
            u[r] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] < 0:
                break
        length = 0
        while j0 >= 0:
            j1 = way[j0]
            p[j0] = r if j1 < 0 else p[j1]
            j0, length = j1, length + 1
        longest = max(longest, length)
    col = np.zeros(nr, np.int64)
    col[p[p >= 0]] = np.nonzero(p >= 0)[0]
    return col, longest, steps


def measurement(b):
    w, h = b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]
    return np.stack([b[..., 0] + w / 2.0, b[..., 1] + h / 2.0, w * h, w / h], -1)


def block_predict(x, P):
    """x [7, ...], P [10, ...] = (a, b, c) of cx, cy, s and pr; in place"""
    x[6] = np.where(x[2] + x[6] <= 0.0, 0.0, x[6])
    for i in range(3):
        a, b, c = P[3 * i].copy(), P[3 * i + 1].copy(), P[3 * i + 2].copy()
        x[i] = x[i] + x[4 + i]
        P[3 * i], P[3 * i + 1], P[3 * i + 2] = ((a + b) + (b + c)) + 1.0, b + c, c + QV[i]
    P[9] = P[9] + 1.0


def block_update(x, P, z):
    """z [4, ...]; in place"""
    for i in range(3):
        a, b, c = P[3 * i].copy(), P[3 * i + 1].copy(), P[3 * i + 2].copy()
        y, S = z[i] - x[i], a + RV[i]
        k0, k1 = a / S, b / S
        x[i], x[4 + i] = x[i] + k0 * y, x[4 + i] + k1 * y
        P[3 * i], P[3 * i + 1], P[3 * i + 2] = a - k0 * a, b - k0 * b, c - k1 * b
    k = P[9] / (P[9] + 10.0)
    x[3] = x[3] + k * (z[3] - x[3])
    P[9] = P[9] - k * P[9]


def state_box(x):
    w = np.sqrt(x[2] * x[3])
    h = x[2] / w
    return np.stack([x[0] - w / 2.0, x[1] - h / 2.0, x[0] + w / 2.0, x[1] + h / 2.0], -1)


def new_filter(z):
    x, P = np.zeros(7), np.zeros(10)
    x[:4] = z
    P[0::3][:3], P[2::3][:3], P[9] = 10.0, 1e4, 10.0
    return x, P


class Tracker:
    """one sequence; `run` takes boxes [F,K,4], count [F] and cls [F,K] or None -> (track_id [F,K] int32, flags [F,K] uint8)"""

    def __init__(self, iou_thres=0.3, max_age=1, min_hits=3, max_tracks=256):
        self.iou_thres, self.max_age, self.min_hits, self.max_tracks = float(iou_thres), int(max_age), int(min_hits), int(max_tracks)
        self.frames = self.next_id = self.dropped = self.longest = self.most_steps = 0
        self.live, self.id, self.cls = np.zeros(SLOTS, bool), np.zeros(SLOTS, np.int64), np.zeros(SLOTS, np.int64)
        self.tsu, self.hits, self.streak = (np.zeros(SLOTS, np.int64) for _ in range(3))
        self.x, self.P = np.zeros((7, SLOTS)), np.zeros((10, SLOTS))
        self.solves = []                                                       # (rows, boxes, longest augmenting path) of every frame

    def costs(self, boxes, good, cls):
        A, B = state_box(self.x)[:, None, :], boxes[None, :, :]
        mx, mn = (lambda a, b: np.where(a > b, a, b)), (lambda a, b: np.where(a < b, a, b))
        iw = mn(A[..., 2], B[..., 2]) - mx(A[..., 0], B[..., 0])
        ih = mn(A[..., 3], B[..., 3]) - mx(A[..., 1], B[..., 1])
        wh = np.where(iw > 0.0, iw, 0.0) * np.where(ih > 0.0, ih, 0.0)
        iou = wh / (((A[..., 2] - A[..., 0]) * (A[..., 3] - A[..., 1]) + (B[..., 2] - B[..., 0]) * (B[..., 3] - B[..., 1])) - wh)
        adm = self.live[:, None] & good[None, :] & (wh > 0.0) & (iou >= self.iou_thres)
        if cls is not None:
            adm &= self.cls[:, None] == cls[None, :]
        g = np.where(adm, iou, 0.0) * 65536.0
        q = np.where(g >= 65535.0, 65535, g.astype(np.int64))
        return np.where(adm, DUMMY - q, DUMMY), adm

    def step(self, boxes, cls=None):
        with np.errstate(all="ignore"):                                        # dead slots and bad boxes hold NaN; the masks drop them
            return self._step(boxes, cls)

    def _step(self, boxes, cls):
        n = len(boxes)
        boxes = np.asarray(boxes, np.float64).reshape(n, 4)
        w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
        good = np.isfinite(boxes).all(1) & (w > 0.0) & (h > 0.0)
        z = measurement(boxes)
        lv = self.live.copy()
        x, P = self.x[:, lv], self.P[:, lv]
        block_predict(x, P)
        self.x[:, lv], self.P[:, lv] = x, P
        self.tsu[lv] += 1
        cost, adm = self.costs(boxes, good, cls)
        rows = np.nonzero(adm.any(1))[0]
        det_slot, slot_det = np.full(n, -1), np.full(SLOTS, -1)
        longest = steps = 0
        if len(rows):
            col, longest, steps = assign(cost[rows])
            for r, c in zip(rows, col):
                if c < n and cost[r, c] < DUMMY:
                    det_slot[c], slot_det[r] = r, c
        self.solves.append((len(rows), n, longest))
        self.longest, self.most_steps = max(self.longest, longest), max(self.most_steps, steps)
        hit = np.nonzero(slot_det >= 0)[0]
        if len(hit):
            x, P = self.x[:, hit], self.P[:, hit]
            block_update(x, P, z[slot_det[hit]].T)
            self.x[:, hit], self.P[:, hit] = x, P
            self.tsu[hit] = 0
            self.hits[hit] += 1
            self.streak[hit] += 1
        miss = lv & (slot_det < 0)
        self.streak[miss] = 0
        self.live[miss & (self.tsu > self.max_age)] = False
        free = [s for s in range(self.max_tracks) if not self.live[s]]
        wants = [j for j in range(n) if good[j] and det_slot[j] < 0]
        for k, (j, s) in enumerate(zip(wants, free)):
            self.x[:, s], self.P[:, s] = new_filter(z[j])
            self.live[s], self.id[s], self.cls[s] = True, self.next_id + k, 0 if cls is None else cls[j]
            self.tsu[s] = self.hits[s] = self.streak[s] = 0
            det_slot[j] = s
        born = min(len(wants), len(free))
        self.next_id, self.dropped = self.next_id + born, self.dropped + len(wants) - born
        tid, flags = np.full(n, -1, np.int32), np.zeros(n, np.uint8)
        for j in range(n):
            s = det_slot[j]
            if s >= 0:
                tid[j] = self.id[s]
                flags[j] = CONFIRMED if self.streak[s] >= self.min_hits or self.frames < self.min_hits else 0
            else:
                flags[j] = DROPPED if good[j] else BAD_BOX
        self.frames += 1
        return tid, flags

    def run(self, boxes, count, cls=None):
        F, K = boxes.shape[:2]
        tid, flags = np.full((F, K), -1, np.int32), np.zeros((F, K), np.uint8)
        for f in range(F):
            n = min(max(int(count[f]), 0), K, SLOTS)
            tid[f, :n], flags[f, :n] = self.step(boxes[f, :n], None if cls is None else cls[f, :n])
        return tid, flags

    def boxes(self):
        """the state boxes of the live slots [live, 4] and their slots"""
        s = np.nonzero(self.live)[0]
        with np.errstate(all="ignore"):
            return state_box(self.x[:, s]), s


@functools.lru_cache(None)
def case(name):
    """the GPU test's cases, seeds chosen on the CPU -> (boxes [S,F,K,4], count [S,F], cls or None, config keywords, a Tracker per
    sequence after its run, track_id [S,F,K], flags [S,F,K])"""
    from mdcv.yolo.track import synthetic_scene
    small, kw = dict(size=(260, 160), K=40), {}
    if name == "a":                      # 12 frames, 20 boxes that cross in a small picture, misses, false positives, frame 5 empty
        scenes = [synthetic_scene(12, 20, 2, empty=(5,), **small)]
    elif name == "b":                    # three sequences of different counts, three classes
        scenes = [synthetic_scene(8, objects, 10 + objects, classes=3, **small) for objects in (5, 17, 30)]
    elif name == "c":                    # more boxes than slots
        scenes, kw = [synthetic_scene(6, 20, 3, size=(400, 300))], dict(max_tracks=8)
    elif name == "d":                    # 200 boxes over fewer tracks; then the first 90 boxes of each frame under ~200 tracks that stay alive
        b, c, _ = synthetic_scene(6, 190, 0, size=(700, 450), miss=0.0, false_pos=10, K=256)
        c[3:] = 90
        scenes, kw = [(b, c, None)], dict(max_age=3, iou_thres=0.1)
    elif name == "e":                    # a bad box of every kind among good ones
        b, c, _ = synthetic_scene(6, 12, 5, size=(260, 160), false_pos=6)
        for f, (j, bad) in enumerate([(0, [np.nan, 0, 9, 9]), (3, [0, 0, np.inf, 9]), (1, [5, 5, 5, 9]), (2, [5, 9, 9, 5]), (4, [-np.inf, 0, 9, 9])]):
            b[f, j] = bad
        scenes = [(b, c, None)]
    boxes, count = np.stack([b for b, _, _ in scenes]), np.stack([c for _, c, _ in scenes])
    cls = None if scenes[0][2] is None else np.stack([k for _, _, k in scenes])
    trackers = [Tracker(**kw) for _ in scenes]
    out = [t.run(boxes[s], count[s], None if cls is None else cls[s]) for s, t in enumerate(trackers)]
    return boxes, count, cls, kw, trackers, np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
