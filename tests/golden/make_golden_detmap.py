"""Writes tests/golden/detmap/cases.npz from the NumPy restatement (tests/helpers/detmap_numpy.py): data only.
  hand::*   the hand-worked example of tests/test_detmap_host.py: two images, seven detections, one class, IoU 0.5, one range
  smoke::*  a small random dataset (4 images, 16 rows, 3 classes of which one is empty, 10 thresholds, 3 ranges) with every expected
            integer and the AP bits: what __graft_entry__.smoke() and the GPU tests check with ==
Run from the repository root: python tests/golden/make_golden_detmap.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import detmap_numpy as DM  # noqa: E402

F = np.float32
SMOKE_RANGES = np.array([[0, np.inf], [0, 200], [200, 1e9]], F)


def hand_case():
    A, B, C, D = (0, 0, 10, 10), (20, 0, 30, 10), (0, 0, 10, 10), (20, 20, 30, 30)
    boxes = np.zeros((2, 4, 4), F)
    prob = np.zeros((2, 4), F)
    boxes[0], prob[0] = [A, (50, 50, 60, 60), B, A], [0.9, 0.8, 0.6, 0.3]
    boxes[1, :3], prob[1, :3] = [C, (40, 0, 50, 10), C], [0.7, 0.5, 0.4]
    return dict(boxes=boxes, prob=prob, count=np.array([4, 3], np.int32), gt_boxes=np.array([[A, B], [C, D]], F),
                gt_count=np.array([2, 2], np.int32))


def main():
    out = {}
    h = hand_case()
    ds = DM.Dataset(4, [0.5], [(0, np.inf)], 1)
    ds.add_pixels(h["boxes"], h["prob"], None, h["count"], h["gt_boxes"], None, h["gt_count"])
    q, tot, ap, err = ds.finalize()
    assert err == 0
    out.update({f"hand::{k}": v for k, v in h.items()})
    out.update({"hand::q": q, "hand::tot": tot, "hand::ap": ap, "hand::status": ds.buffers()[3]})

    rng = np.random.default_rng(2025)
    b = DM.random_batch(rng, 4, 16, 6, 3, empty_images=False)
    ds = DM.Dataset(16, DM.COCO_THRESHOLDS, SMOKE_RANGES, 3)
    ds.add_pixels(**b)
    q, tot, ap, err = ds.finalize()
    assert err == 0 and (ap[:2, 0, 0] > 0).all() and (ap[2] == -1).all()
    out.update({f"smoke::{k}": v for k, v in b.items()})
    out.update({"smoke::thresholds": np.array(DM.COCO_THRESHOLDS, F), "smoke::ranges": SMOKE_RANGES, "smoke::q": q, "smoke::tot": tot,
                "smoke::ap": ap, "smoke::status": ds.buffers()[3], "smoke::n_gt": ds.n_gt})
    os.makedirs(os.path.join(HERE, "detmap"), exist_ok=True)
    path = os.path.join(HERE, "detmap", "cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; hand AP", ap if False else out["hand::ap"].ravel(), "smoke AP50", out["smoke::ap"][:, 0, 0])


if __name__ == "__main__":
    main()
