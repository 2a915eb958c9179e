"""Batched RektNet validation: the reference's `eval_model` and `print_kpt_L2_distance` (RektNet/train_eval.py:115-186) without the
batch-1 loop.

The reference validates with `DataLoader(val_dataset, batch_size=1)` (train_eval.py:258) and reads three `.item()` per image.  What it
reports is therefore the mean over the images of the loss of every image ALONE.  That is not what `CrossRatioLoss` returns for a batch:
its geometric term is the mean of a [B,B] all-pairs matrix (cross_ratio_loss.py:36-57), a per-image quantity only at B = 1 (DESIGN §18
has the figures).  `KeypointEvaluator` keeps the reference's meaning at any batch size: samples are packed into chunks, a chunk costs one
eval-mode forward and one `mdcv_kpt_eval_rows` launch (csrc/kpt_eval.hip: per-sample loss triples and per-key-point pixel distances), and
nothing is read back before a result is asked for.

    ev = KeypointEvaluator(model, loss_function, input_size)
    for x, y_hm, y_pts, names, sizes in loader:          # any batch size; CPU or device tensors
        ev.add(x, y_hm, y_pts, names, sizes)
    val_loc, val_geo, val_loss = ev.losses()             # eval_model's triple
    final_stats, total_dist, final_stats_std = ev.distances()

`eval_model` and `print_kpt_L2_distance` below have the reference's signatures, prints and files.  No CPU fallback.
"""
import os

import numpy as np
import torch

from .. import _lib
from .cross_ratio_loss import _TYPES

ROW = 12                                   # MDCV_KPT_EVAL_ROW: loc, geo, total, d0..d6, 0, 0
NUM_KPT = 7


def loss_sums(rows):
    """eval_model's arithmetic on the read-back rows [N, >= 3] (train_eval.py:119-135): `+= .item()` in sample order, which is float64
    addition of fp32 values, then `/ batch_num`.  No rows: ZeroDivisionError, as the reference's 0 / 0."""
    sums = [0, 0, 0]
    n = 0
    for r in np.asarray(rows, np.float32):
        sums[0] += float(r[0])
        sums[1] += float(r[1])
        sums[2] += float(r[2])
        n += 1
    return sums[0] / n, sums[1] / n, sums[2] / n


def distance_stats(dist):
    """utils.calculate_mean_distance (utils.py:246-287) on the fp32 distances [N, 7]: per key point `np.mean` / `np.std` of a float32 list
    (population std), and their left-to-right float32 sum.  -> (final_stats[7], total_dist, final_stats_std[7])"""
    dist = np.asarray(dist, np.float32).reshape(-1, NUM_KPT)
    cols = [np.ascontiguousarray(dist[:, k]) for k in range(NUM_KPT)]
    std = [np.std(c) for c in cols]
    mean = [np.mean(c) for c in cols]
    total = mean[0]
    for m in mean[1:]:
        total = total + m
    return mean, total, std


def _pair(input_size):
    if isinstance(input_size, (tuple, list)):
        return float(input_size[0]), float(input_size[1])
    return float(input_size), float(input_size)


def _per_sample_sizes(sizes, count):
    """-> [(h, w)] * count from what a loader hands over as `image.shape`: the default collate's three [B] tensors (h, w, c), or one
    (h, w, c) per sample"""
    if len(sizes) == 3 and all(torch.is_tensor(s) and s.dim() == 1 for s in sizes):
        h, w = sizes[0].tolist(), sizes[1].tolist()
        out = list(zip(h, w))
    else:
        out = [(int(s[0]), int(s[1])) for s in sizes]
    if len(out) != count:
        raise ValueError(f"KeypointEvaluator.add: {len(out)} sizes for {count} samples")
    return [(int(h), int(w)) for h, w in out]


class KeypointEvaluator:
    """Per-sample validation of a KeypointNet over batches of any size (module docstring).

    `loss_function`: a CrossRatioLoss (its loss_type, include_geo and gammas are read), or None when only distances are wanted.
    `input_size`: S or (S0, S1), the factors of the pixel distances: d_k = |(3 S0 (px - tx), 3 S1 (py - ty))|.  The 3 is the reference's own
    factor, `x_batch.shape[1]` (train_eval.py:152-157).  `chunk`: images per forward; the tail chunk is padded with zero images so that one
    launch plan serves the whole run (eval-mode BatchNorm keeps samples independent) and the kernel is given the real count only.
    `y_hm` is staged only for `l2_heatmap` and may be None otherwise."""

    def __init__(self, model, loss_function, input_size, chunk=256):
        self.model, self.chunk = model, int(chunk)
        if not 1 <= self.chunk <= 65535:
            raise ValueError("KeypointEvaluator: chunk must be in 1..65535")
        if loss_function is None:
            self.loss_type, self.include_geo, self.gamma = 0, 0, (0.0, 0.0)
        else:
            if loss_function.loss_type not in _TYPES:
                raise ValueError(f"KeypointEvaluator: unknown loss type {loss_function.loss_type!r}")
            self.loss_type = _TYPES[loss_function.loss_type]
            self.include_geo = int(bool(loss_function.include_geo))
            self.gamma = (float(loss_function.geo_loss_gamma_horz), float(loss_function.geo_loss_gamma_vert))
        self.has_loss = loss_function is not None
        s0, s1 = _pair(input_size)
        self.dist_scale = (3.0 * s0, 3.0 * s1)
        self.device = next(model.parameters()).device
        self.n = 0                                   # rows written
        self._fill = 0                               # samples waiting in the staging buffers
        self._x = self._pts = self._hm = self._rows = self._host = None
        self.names, self._sizes = [], []

    # ------------------------------------------------------------------ feeding
    def add(self, x, y_hm, y_pts, names=None, sizes=None):
        _lib.require_gpu()
        dev = self.device
        x = x.detach().to(device=dev, dtype=torch.float32, non_blocking=True)
        y_pts = y_pts.detach().to(device=dev, dtype=torch.float32, non_blocking=True)
        count = x.shape[0]
        if tuple(y_pts.shape) != (count, NUM_KPT, 2):
            raise ValueError(f"KeypointEvaluator.add: points of shape {tuple(y_pts.shape)} for {count} images; the kernel takes [B, 7, 2]")
        if self.loss_type == 1:
            if y_hm is None:
                raise ValueError("KeypointEvaluator.add: l2_heatmap needs the target heat-maps")
            y_hm = y_hm.detach().to(device=dev, dtype=torch.float32, non_blocking=True)
            if y_hm.shape[0] != count or y_hm.shape[1] != NUM_KPT:
                raise ValueError(f"KeypointEvaluator.add: heat-maps of shape {tuple(y_hm.shape)} for {count} images")
        if self._x is None:
            self._x = torch.zeros((self.chunk,) + tuple(x.shape[1:]), dtype=torch.float32, device=dev)
            self._pts = torch.zeros(self.chunk, NUM_KPT, 2, dtype=torch.float32, device=dev)
            if self.loss_type == 1:
                self._hm = torch.zeros((self.chunk,) + tuple(y_hm.shape[1:]), dtype=torch.float32, device=dev)
        if names is not None:
            self.names.extend(names)
        if sizes is not None:
            self._sizes.extend(_per_sample_sizes(sizes, count))
        self._host = None
        off = 0
        while off < count:
            take = min(self.chunk - self._fill, count - off)
            lo, hi = self._fill, self._fill + take
            self._x[lo:hi].copy_(x[off:off + take])
            self._pts[lo:hi].copy_(y_pts[off:off + take])
            if self._hm is not None:
                self._hm[lo:hi].copy_(y_hm[off:off + take])
            self._fill, off = hi, off + take
            if self._fill == self.chunk:
                self._flush()

    def _grow(self, need):
        if self._rows is None or self._rows.shape[0] < need:
            cap = max(need, 4 * self.chunk, 2 * (self._rows.shape[0] if self._rows is not None else 0))
            rows = torch.empty(cap, ROW, dtype=torch.float32, device=self.device)
            if self.n:
                rows[:self.n].copy_(self._rows[:self.n])
            self._rows = rows

    def _flush(self):
        """one eval-mode, no-grad forward of the staged chunk, one kernel call on its real samples"""
        count = self._fill
        if count == 0:
            return
        if count < self.chunk:
            self._x[count:].zero_()                  # the padded tail: zero images
        was = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                hm, pts = self.model(self._x)
        finally:
            self.model.train(was)
        self._grow(self.n + count)
        self.eval_rows(hm, pts, self._hm, self._pts, count, self._rows[self.n:])
        self.n += count
        self._fill = 0

    def eval_rows(self, hm, pts, thm, tpts, count, out):
        """mdcv_kpt_eval_rows on the first `count` samples with this evaluator's settings; `out` [>= count, 12] fp32 on the device"""
        L = _lib.lib()
        H, W = (int(hm.shape[2]), int(hm.shape[3])) if self.loss_type == 1 else (0, 0)
        if self.loss_type == 1:
            if tuple(thm.shape[1:]) != tuple(hm.shape[1:]):
                raise ValueError(f"KeypointEvaluator: target heat-maps {tuple(thm.shape[1:])}, the model's are {tuple(hm.shape[1:])}")
            hm, thm = hm.contiguous(), thm.contiguous()
        pts = pts.contiguous()
        with torch.cuda.device(self.device):
            L.check(L.kpt_eval_rows(hm.data_ptr() if self.loss_type == 1 else None, pts.data_ptr(),
                                    thm.data_ptr() if self.loss_type == 1 else None, tpts.data_ptr(), count, H, W, self.loss_type,
                                    self.include_geo, self.gamma[0], self.gamma[1], self.dist_scale[0], self.dist_scale[1], out.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream), "kpt_eval_rows")

    # ------------------------------------------------------------------ results
    def rows(self):
        """the device tensor [N, 12]: loc, geo, total, d0..d6, 0, 0 per sample, in the order the samples were added"""
        self._flush()
        if self._rows is None:
            return torch.empty(0, ROW, dtype=torch.float32, device=self.device)
        return self._rows[:self.n]

    def _read(self):
        if self._host is None:
            self._host = self.rows().cpu().numpy()           # the one read-back
        return self._host

    def losses(self):
        """(val_loc_loss, val_geo_loss, val_loss) as eval_model computes them (train_eval.py:119-135)"""
        if not self.has_loss:
            raise ValueError("KeypointEvaluator.losses: built without a loss function")
        return loss_sums(self._read())

    def distances(self):
        """(final_stats[7], total_dist, final_stats_std[7]) as utils.calculate_mean_distance returns them (utils.py:246-287)"""
        return distance_stats(self._read()[:, 3:3 + NUM_KPT])

    def image_sizes(self):
        """[(h, w)] of the samples whose loader handed sizes over"""
        return list(self._sizes)


def eval_model(model, dataloader, loss_function, input_size):
    """The reference's eval_model (train_eval.py:115-138): same signature, same two printed lines, same return triple, and the model is
    left in eval mode.  The losses are PER SAMPLE, whatever the loader's batch size: the mean over the images of CrossRatioLoss on each
    image alone, which is what the reference computes with the batch_size=1 loader it builds (train_eval.py:258).  An empty loader raises
    ZeroDivisionError, as there."""
    print("\tStarting validation...")
    model.eval()
    ev = KeypointEvaluator(model, loss_function, input_size)
    for x_batch, y_hm_batch, y_point_batch, image_name, _ in dataloader:
        ev.add(x_batch, y_hm_batch, y_point_batch)
    val_loc_loss, val_geo_loss, val_loss = ev.losses()
    print(f"\tValidation: MSE/Geometric/Total Loss: {round(val_loc_loss,10)}/{round(val_geo_loss,10)}/{round(val_loss,10)}")
    return val_loc_loss, val_geo_loss, val_loss


def print_kpt_L2_distance(model, dataloader, kpt_keys, study_name, evaluate_mode, input_size):
    """The reference's print_kpt_L2_distance (train_eval.py:140-186): same prints, `logs/<study_name>.txt` holds `total_dist`, and with
    `evaluate_mode` one `[width, height]:sum` line per image is appended to `logs/rektnet_validation.txt` from the loader's sizes.
    The forward runs in eval mode without gradients and the model's training flag is put back.  The reference calls `model(x_batch)` as
    the model stands, but only ever reaches this function after eval_model has left the model in eval mode (train_eval.py:82, 284-291).
    `logs/` is created if it is missing."""
    ev = KeypointEvaluator(model, None, input_size)
    for x_batch, y_hm_batch, y_point_batch, _, image_shape in dataloader:
        ev.add(x_batch, None, y_point_batch, sizes=image_shape if evaluate_mode else None)
    final_stats, total_dist, final_stats_std = ev.distances()
    os.makedirs("logs", exist_ok=True)
    if evaluate_mode:
        dist = ev._read()[:, 3:3 + NUM_KPT]
        with open("logs/rektnet_validation.txt", "a") as validation_textfile:
            for (height, width), kpt_dis in zip(ev.image_sizes(), dist):
                kpt_dis = list(kpt_dis)
                print(width, height)
                print(kpt_dis)
                single_img_kpt_dis_sum = sum(kpt_dis)
                validation_textfile.write(f"{[width, height]}:{single_img_kpt_dis_sum}\n")
    print(f'Mean distance error of each keypoint is:')
    for i, kpt_key in enumerate(kpt_keys):
        print(f'\t{kpt_key}: {final_stats[i]}')
    print(f'Standard deviation of each keypoint is:')
    for i, kpt_key in enumerate(kpt_keys):
        print(f'\t{kpt_key}: {final_stats_std[i]}')
    print(f'Total distance error is: {total_dist}')
    with open("logs/" + study_name + ".txt", "w") as result:
        result.write(str(total_dist))
