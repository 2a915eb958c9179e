"""CPU: the host half of dataset preparation (mdcv/data/prep.py) and the NumPy + math.fsum restatement of the anchor k-means
(tests/helpers/anchor_refs.py) against what the reference's own functions computed (tests/golden/anchors.npz, written by
tests/golden/make_golden_anchors.py).  The kernel is compared with the same restatement in tests/test_gpu_anchors.py."""
import csv
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import anchor_refs as ar  # noqa: E402
from anchor_cases import host_kmeans, write_raw_dataset  # noqa: E402

from mdcv.data import prep  # noqa: E402
from mdcv.data.images.labels import read_label_csv  # noqa: E402
from mdcv.yolo.models import _read_anchor_row  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "anchors.npz"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------ the k-means
@pytest.mark.parametrize("i", range(4))
def test_dyadic_bit_equal(gold, i):
    """every sum of the dyadic set is exact in any order, so the reference's pairwise mean IS fl(exact sum / n): bits, assignment, count"""
    pts = gold["dyadic::points"]
    assert ar.draws(int(gold["dyadic::seeds"][i]), len(pts), 9) == gold["dyadic::init"][i].tolist()
    got = ar.lloyd(pts, gold["dyadic::init"][i])
    assert got["iterations"] == int(gold["dyadic::iterations"][i])
    assert np.array_equal(got["assign"], gold["dyadic::assign"][i])
    assert np.array_equal(bits(got["centroids"]), bits(gold["dyadic::centroids"][i]))
    assert not got["nan"]


@pytest.mark.parametrize("i", range(4))
def test_generic_within_pairwise_bound(gold, i):
    """same assignment and count; every centroid within the bound of the reference's own pairwise summation, cluster by cluster"""
    pts = gold["generic::points"]
    assert ar.draws(int(gold["generic::seeds"][i]), len(pts), 9) == gold["generic::init"][i].tolist()
    got = ar.lloyd(pts, gold["generic::init"][i])
    assert got["iterations"] == int(gold["generic::iterations"][i])
    assert np.array_equal(got["assign"], gold["generic::assign"][i])
    ref = gold["generic::centroids"][i]
    for k in range(9):
        members = pts[got["assign"] == k]
        for j in range(2):
            bound = ar.pairwise_mean_bound(members[:, j])
            err = abs(float(got["centroids"][k, j]) - float(ref[k, j]))
            print(f"seed {i} cluster {k} coord {j}: |diff| {err:.3e} bound {bound:.3e} ulp {err / math.ulp(float(ref[k, j])):.1f}")
            assert err <= bound


def test_repeated_index_nan_cluster(gold):
    pts = gold["dyadic::points"]
    got = ar.lloyd(pts, gold["repeat::init"][0])
    ref = gold["repeat::centroids"][0]
    assert np.isnan(ref).any(axis=1).tolist() == [False, False, True, False]
    assert np.array_equal(np.isnan(got["centroids"]), np.isnan(ref)) and got["nan"]
    alive = ~np.isnan(ref).any(axis=1)
    assert np.array_equal(bits(got["centroids"][alive]), bits(ref[alive]))
    assert np.array_equal(got["assign"], gold["repeat::assign"][0])
    assert got["iterations"] == int(gold["repeat::iterations"][0])


def test_equal_roots_keep_the_lower_index():
    pts, init = ar.equal_root_case()
    idx, q = ar.assign(pts, pts[init])
    q_to_0 = (pts[2, 0] - pts[0, 0]) ** 2 + (pts[2, 1] - pts[0, 1]) ** 2
    q_to_1 = (pts[2, 0] - pts[1, 0]) ** 2 + (pts[2, 1] - pts[1, 1]) ** 2
    assert q_to_0 > q_to_1 and math.sqrt(q_to_0) == math.sqrt(q_to_1)
    assert idx.tolist() == [0, 1, 0] and q[2] == q_to_0


def test_nan_centroid_never_wins_and_first_minimum_wins():
    pts = np.array([[0.0, 0.0], [2.0, 0.0], [1.0, 0.0]])
    idx, _ = ar.assign(pts, np.array([[np.nan, np.nan], [0.0, 0.0], [2.0, 0.0]]))
    assert idx.tolist() == [1, 2, 1]                       # box 2 is at distance 1 from both: the first of them


def test_restart_selection():
    big = 1 << 70
    assert ar.select_best([big + 5, big + 3, big + 3, big + 9], [False] * 4) == 1          # tie: the lowest index
    assert ar.select_best([1, big, big + 1], [True, False, False]) == 1                       # a NaN restart never wins
    assert ar.select_best([3, 2], [True, True]) is None
    for d, n in (([5, 5, 4], [False, False, True]), ([big, big - 1], [False, False])):
        assert prep.select_best(d, n) == ar.select_best(d, n)


def test_initial_indices_are_the_references_draws(gold):
    n = len(gold["dyadic::points"])
    idx = prep.initial_indices(n, 9, 2, 3)
    assert idx.shape == (3, 9) and idx.reshape(-1).tolist() == ar.draws(2, n, 27)
    assert idx[0].tolist() == gold["dyadic::init"][2].tolist()


@pytest.mark.parametrize("bad,word", [(np.nan, "not finite"), (np.inf, "not finite"), (16384.0, "2^14"), (-16384.0, "2^14"),
                                      (2.0 ** -65, "2^-64"), (2.0 ** -40 + 2.0 ** -70, "2^-64"), (-3 * 2.0 ** -65, "2^-64")])
def test_refused_coordinates_name_the_box(bad, word):
    pts = np.full((7, 2), 12.5)
    pts[4, 1] = bad
    pts[6, 0] = np.nan
    with pytest.raises(ValueError, match="box 4") as e:
        prep.kmeans_anchors(pts, 2)
    assert word in str(e.value)


def test_accepted_coordinates():
    pts = np.array([[16383.999999999998, -(2.0 ** -64)], [0.0, -0.0], [-16383.5, 2.0 ** -64 * 3]])
    assert prep.check_boxes(pts).shape == (3, 2)


def test_refused_shapes():
    pts = np.ones((5, 2))
    with pytest.raises(ValueError, match="num_clst"):
        prep.kmeans_anchors(pts, 17)
    with pytest.raises(ValueError, match="num_clst"):
        prep.kmeans_anchors(pts, 0)
    with pytest.raises(ValueError, match="N"):
        prep.kmeans_anchors(np.zeros((0, 2)), 2)
    with pytest.raises(ValueError, match="restarts"):
        prep.kmeans_anchors(pts, 2, restarts=65)
    with pytest.raises(ValueError, match="init"):
        prep.kmeans_anchors(pts, 2, init=[[0, 5]])
    with pytest.raises(ValueError, match="shape"):
        prep.kmeans_anchors(np.ones((5, 3)), 2)


# ----------------------------------------------------------------------------------------------------- scales, splits, files
def main_inputs(gold):
    """the recorded run's input as prepare_dataset groups it: {(img_h, img_w): [(h, w)]} in first-seen order"""
    box_dict = {}
    for (W, H), (h, w) in zip(gold["main::sizes"].tolist(), gold["main::hw"].tolist()):
        box_dict[(H, W)] = box_dict.get((H, W), []) + [(h, w)]
    return box_dict


def test_scales_against_the_recorded_run(gold):
    scale, hs, ws = prep.camera_scales(main_inputs(gold))
    assert np.array_equal(gold["main::wh_cols"], gold["main::sizes"])
    got = np.array([scale[(H, W)] for W, H in gold["main::sizes"].tolist()])
    assert np.array_equal(bits(got), bits(gold["main::scale"]))
    assert all(type(s) is float for s in scale.values())


def test_percentile_picks_with_ties_against_the_recorded_anchors(gold):
    """twelve heights over 230 boxes: which (h, w) the stable sort leaves at the two percentile positions decides min_w, and min_w shifts every
    scaled width by a multiple of the ratio (>= 6.6).  The reference's anchors.txt (two decimals) after np.random.seed(0) shows the shift."""
    _, hs, ws = prep.camera_scales(main_inputs(gold))
    pts = np.array([hs, ws]).T
    got = ar.lloyd(pts, ar.draws(0, len(pts), 9))
    text = [[float('%0.2f' % c[0]), float('%0.2f' % c[1])] for c in got["centroids"]]
    assert text == gold["main::anchors_txt"].tolist()


def test_percentile_picks_by_hand():
    group = [(5, 50), (3, 30), (5, 51), (3, 31), (9, 90), (1, 10)] + [(5, 52 + i) for i in range(14)]       # n = 20
    scale, hs, ws = prep.camera_scales({(48, 64): group}, max_cone=83, min_cone=10)
    # stable by h: (1,10) (3,30) (3,31) (5,50) (5,51) (5,52).. (5,65) (9,90); max = [int(19.0) - 1] = [18] = (5,65), min = [1] = (3,30)
    r = (83 - 10) / (5 - 3)
    assert scale == {(48, 64): r}
    assert hs == [(h - 3) * r + 10 for h, _ in group] and ws == [(w - 30) * r + 10 for _, w in group]
    with pytest.raises(ZeroDivisionError):
        prep.camera_scales({(1, 1): [(4, 2), (4, 3), (4, 9)]})


def test_percentile_two_boxes_raise():
    with pytest.raises(ZeroDivisionError):                                   # n = 2: max = sorted[int(1.9) - 1] = sorted[0] = min
        prep.camera_scales({(1, 1): [(4, 2), (6, 3)]})


def rows_of(gold):
    scale, _, _ = prep.camera_scales(main_inputs(gold))
    rows = []
    for name, (W, H), (h, w) in zip(gold["main::names"].tolist(), gold["main::sizes"].tolist(), gold["main::hw"].tolist()):
        rows.append([name, "http://x/" + name, W, H, scale[(H, W)], str(h), str(w)])
    return rows


def test_split_against_the_recorded_run(gold):
    """the reference's run had no box-less row, so its trade moved every labelled training row to validate.csv: reference_trade=True"""
    split = prep.split_rows(rows_of(gold), (75, 15, 0), reference_trade=True)
    for fn in prep.FILES:
        assert [r[0] for r in split[fn]] == gold["main::" + fn].tolist(), fn
    assert split["traded"] == 0 and split["train.csv"] == []


def test_split_without_boxless_rows_trades_nothing(gold):
    rows = rows_of(gold)
    split = prep.split_rows(rows, (75, 15, 0))
    assert [r[0] for r in split["train.csv"]] == [r[0] for i, r in enumerate(rows) if i % 100 < 75]
    assert [r[0] for r in split["validate.csv"]] == [r[0] for i, r in enumerate(rows) if 75 <= i % 100 < 90]
    assert [r[0] for r in split["test.csv"]] == [r[0] for i, r in enumerate(rows) if i % 100 >= 90]
    assert split["train-validate.csv"] == [r for i, r in enumerate(rows) if i % 100 < 90] and split["all.csv"] == rows


def test_trade_by_hand():
    """10 rows split 6-3-1: validate = rows 6, 7, 8.  Rows 1 and 7 have no box.  Row 7 leaves validate for the END of train; the FIRST
    labelled training row (row 0) goes to the end of validate.  Both trades agree as soon as one row is traded."""
    rows = [[f"n{i}", "u", 64, 48, 2.5, "" if i in (1, 7) else "[1, 2, 3, 4]", ""] for i in range(10)]
    s = prep.split_rows([list(r) for r in rows[:10]], (6, 3, 1))
    assert [r[0] for r in s["train.csv"]] == ["n1", "n2", "n3", "n4", "n5", "n7"]
    assert [r[0] for r in s["validate.csv"]] == ["n6", "n8", "n0"]
    assert [r[0] for r in s["test.csv"]] == ["n9"] and s["traded"] == 1
    assert [r[0] for r in s["train-validate.csv"]] == [f"n{i}" for i in range(9)] and len(s["all.csv"]) == 10
    assert prep.split_rows([list(r) for r in rows[:10]], (6, 3, 1), reference_trade=True) == s
    # i % 100 over more than a hundred rows: rows 100..102 are training rows again; rows 5 and 80 have no box
    rows = [[f"m{i}", "u", 64, 48, 2.5, "" if i in (5, 80) else "[1, 2, 3, 4]"] for i in range(103)]
    s = prep.split_rows(rows, (75, 15, 0))
    assert [r[0] for r in s["train.csv"]] == [f"m{i}" for i in list(range(1, 75)) + [100, 101, 102, 80]]
    assert [r[0] for r in s["validate.csv"]] == [f"m{i}" for i in list(range(75, 80)) + list(range(81, 90)) + [0]]
    assert [r[0] for r in s["test.csv"]] == [f"m{i}" for i in range(90, 100)] and s["traded"] == 1


def test_header_rows_and_round_trip(gold, tmp_path):
    cents = np.array([[30.5, 12.25], [10.1, 7.3], [1e-3, 2e22], [83.0, 41.000000000000014]])
    rows = [["a.png", "u", 64, 48, 6.636363636363637, "[1, 2, 30, 11]", "", "[4.5, 0, 7, 3]"], ["b.png", "u", 40, 56, 7.3, "", ""]]
    split = {fn: rows for fn in prep.FILES}
    prep.write_csvs(str(tmp_path), split, prep.anchor_row(cents, "wh"))
    with open(tmp_path / "validate.csv", newline="") as f:
        got = list(csv.reader(f))
    assert got[0] == gold["main::head_note"].tolist() and got[1] == gold["main::second_row"].tolist()
    with open(tmp_path / "train.csv", newline="") as f:
        raw = f.read()
    assert raw.split("\r\n")[0] == '"' + prep.anchor_row(cents, "wh") + '"'
    order = sorted(range(4), key=lambda k: cents[k, 0] * cents[k, 1])
    assert _read_anchor_row(str(tmp_path / "train.csv")) == [[float(cents[k, 1]), float(cents[k, 0])] for k in order]
    prep.write_csvs(str(tmp_path), split, prep.anchor_row(cents, "hw"))
    assert _read_anchor_row(str(tmp_path / "train.csv")) == [[float(cents[k, 0]), float(cents[k, 1])] for k in order]
    back = read_label_csv(str(tmp_path / "train.csv"), "imgs")
    assert [(r[0], r[1], r[2], r[3]) for r in back] == [(os.path.join("imgs", "a.png"), 64, 48, 6.636363636363637),
                                                       (os.path.join("imgs", "b.png"), 40, 56, 7.3)]
    assert back[0][4].tolist() == [[1, 2, 30, 11], [4.5, 0, 7, 3]] and back[1][4].shape == (0, 4)


def test_anchor_row_text():
    assert prep.anchor_row([[2.0, 3.0], [1.0, 0.1]], "hw") == "1.0, 0.1|2.0, 3.0"
    assert prep.anchor_row(np.array([[2.0, 3.0], [1.0, 0.1]]), "wh") == "0.1, 1.0|3.0, 2.0"
    with pytest.raises(ValueError):
        prep.anchor_row([[1.0, 1.0]], "xy")


# ------------------------------------------------------------------------------------------------- prepare_dataset on the host
def test_prepare_dataset_on_the_host(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(prep, "kmeans_anchors", host_kmeans)
    src, images = write_raw_dataset(str(tmp_path))
    out = str(tmp_path / "out")
    km = prep.prepare_dataset(src, images, out, num_clst=3, if_plot=True, restarts=2)
    assert "if_plot" in capsys.readouterr().out
    assert sorted(os.listdir(out)) == sorted(prep.FILES + ("anchors.txt",))
    raw = prep.read_raw_labels(src, images)
    assert [len(r[3]) for r in raw] == [2, 2, 2, 0, 2, 3, 2, 2, 2, 2, 2, 2] and (raw[0][1], raw[0][2]) == (96, 64)
    rows = read_label_csv(os.path.join(out, "train.csv"), images)
    assert len(rows) == 12 and [len(r[4]) for r in rows] == [len(r[3]) for r in raw]
    assert [(r[1], r[2]) for r in rows[:2]] == [(96, 64), (80, 112)]
    scale, hs, ws = prep.camera_scales({(64, 96): sum((r[3] for r in raw[0::2]), []), (112, 80): sum((r[3] for r in raw[1::2]), [])})
    assert [r[3] for r in rows] == [scale[(64, 96)], scale[(112, 80)]] * 6
    order = sorted(range(3), key=lambda k: km.centroids[k, 0] * km.centroids[k, 1])
    assert _read_anchor_row(os.path.join(out, "train.csv")) == [[float(km.centroids[k, 1]), float(km.centroids[k, 0])] for k in order]
    with open(os.path.join(out, "anchors.txt")) as f:
        assert f.read() == "".join('%0.2f,%0.2f \n' % (c[0], c[1]) for c in km.centroids)
    with open(os.path.join(out, "all.csv"), newline="") as f:
        all_rows = list(csv.reader(f))
    assert all_rows[2 + 4][5:] == raw[4][0][2:] and "" in all_rows[2 + 4][5:]
    # the command line does the same
    out2 = str(tmp_path / "out2")
    prep.main(["--input_csvs", src, "--dataset_path", images, "--output_path", out2, "--num_clst", "3", "--restarts", "2", "--no_if_plot"])
    for fn in prep.FILES + ("anchors.txt",):
        with open(os.path.join(out, fn), "rb") as a, open(os.path.join(out2, fn), "rb") as b:
            assert a.read() == b.read(), fn
    prep.main(["--input_csvs", src, "--dataset_path", images, "--output_path", out2, "--num_clst", "3", "--anchor_order", "hw", "--seed", "4"])
    assert _read_anchor_row(os.path.join(out2, "train.csv")) != _read_anchor_row(os.path.join(out, "train.csv"))


def test_prepare_dataset_refusals(tmp_path, monkeypatch):
    monkeypatch.setattr(prep, "kmeans_anchors", host_kmeans)
    src, images = write_raw_dataset(str(tmp_path))
    os.remove(os.path.join(images, "f7.png"))
    with pytest.raises(FileNotFoundError, match="f7.png"):
        prep.prepare_dataset(src, images, str(tmp_path / "o"), num_clst=3)
    with pytest.raises(ValueError, match="anchor_order"):
        prep.prepare_dataset(src, images, str(tmp_path / "o"), anchor_order="xy")
