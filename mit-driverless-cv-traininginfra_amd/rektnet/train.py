"""The native form of the reference's RektNet `train_model` (train_eval.py:45-113).

Same signature, `EPOCH n` / `Training:` lines, per-batch descriptions, best-loss and tolerance bookkeeping, `.pt` checkpoints and stop
message; validation is the batched `eval_model` (evaluate.py).  The three `.item()` reads per step are one HIP launch (`mdcv.trainlog`,
csrc/train_log.hip): a batch's description is formatted when its row has landed on the host, the epoch's sums are added on the device in
the reference's order, and the loop waits for the GPU once per epoch.  The ONNX branch (train_eval.py:92-99) is skipped with a notice.
"""
import contextlib
import os

import torch

from .. import trainlog
from .evaluate import eval_model


def format_batch_description(batch_num, loc_loss, geo_loss, loss):
    """the tqdm description of train_eval.py:75 from the step's three numbers (`geo_loss` is the int 0 without include_geo, as there)"""
    return f"Batch {batch_num}. Location Loss: {round(loc_loss,5)}. Geo Loss: {round(geo_loss,5)}. Total Loss: {round(loss,5)}"


def format_epoch_line(total_loss, batch_num):
    """the `Training:` line of train_eval.py:81 from the epoch's three sums; no batches: ZeroDivisionError, as there"""
    return f"\tTraining: MSE/Geometric/Total Loss: {round(total_loss[0]/batch_num,10)}/{round(total_loss[1]/batch_num,10)}/{round(total_loss[2]/batch_num,10)}"


def _host_number(t):
    """a loss the loss function computed on the HOST (CrossRatioLoss's `torch.tensor(0)` without include_geo): its `.item()` costs no GPU wait"""
    return t.item() if torch.is_tensor(t) else t


def train_model(model, output_uri, dataloader, loss_function, optimizer, scheduler, epochs, val_dataloader, intervals, input_size, num_kpt,
                save_checkpoints, kpt_keys, study_name, evaluate_mode, progress=None, log=print, ring=64, stats=None, guard=None,
                clip_grad_norm=0.0, skip_nonfinite=False, ema=None, ema_decay=0.0, ema_warmup=10, augment=None):
    """train_eval.py:45-113.  `progress(description)` gets every batch's description (default: dropped, a bar's text has no other
    reader), `log(line)` every printed line; `stats`, a dict, receives `host_waits` (per epoch, a list).  Batches already on the device
    (ConeCropBatches, SyntheticCones) are consumed as they are, host batches through `trainlog.prefetch`.  The heat-map targets are only
    moved for `l2_heatmap`-style losses by the loss function itself; `optimizer` may be any torch optimizer (FusedAdam for the headline
    rate).

    `guard`: the `mdcv.optim.GradGuard` to report on; default: the one the optimizer holds.  `clip_grad_norm` > 0 / `skip_nonfinite` (this
    module has no command line: keywords, as `--clip_grad_norm` / `--skip_nonfinite` of mdcv.yolo.train) give a FusedAdam / FusedSGD
    that holds no guard one with those settings; an optimizer that cannot take a guard is a TypeError.  With a guard, one line follows
    each epoch's `Training:` line, from one read of the guard's counters after the epoch's wait:
    `train Epoch: 3, grad norm max 41.2 mean 7.9, clipped 12, skipped 1 of 240 steps`.  Without one: no line, no read.

    `ema`: the `mdcv.optim.WeightEMA` to validate with; default: the one the optimizer holds.  `ema_decay` > 0 (with `ema_warmup`) gives a
    FusedAdam / FusedSGD that holds none a `WeightEMA(model, ema_decay, ema_warmup)`; an optimizer that cannot take one is a TypeError.
    (An `ema` handed over beside an optimizer that does not hold it -- a torch optimizer -- is updated by this loop after each `step()`.)
    With an EMA, `eval_model` runs with the averaged weights and BatchNorm statistics swapped in, so `val_loss`, the best
    epoch and the tolerance describe the averaged model; the `.pt` checkpoint keeps the live `'model'` and gains `'ema'` (the EMA's
    `state_dict()`).  Without one nothing changes.

    `augment`: a dict of `mdcv.data.KeypointAugBatches` keywords (an empty one: its defaults) wraps `dataloader` -- the TRAINING loader,
    never `val_dataloader` -- in one (affine, flip and colour on the device, one launch per batch); a `dataloader` that
    already is a `KeypointAugBatches` is used as it is.  Either way one line follows each epoch's `Training:` line (behind the guard's, if
    there is one), from one read of the wrapper's counters after the epoch's wait:
    `train Epoch: 3, key-point augmentation: 951 of 1024 images augmented, rejected 73, passed through 0`.  Without: no line, no launch."""
    from ..data.kptaug import KeypointAugBatches
    if augment is not None and not isinstance(dataloader, KeypointAugBatches):
        dataloader = KeypointAugBatches(dataloader, **augment)
    kptaug = dataloader if isinstance(dataloader, KeypointAugBatches) else None
    if guard is None:
        guard = getattr(optimizer, "guard", None)
    if guard is None and (clip_grad_norm > 0 or skip_nonfinite):
        from ..optim import GradGuard, _FlatOptimizer
        if not isinstance(optimizer, _FlatOptimizer):
            raise TypeError("clip_grad_norm / skip_nonfinite need a FusedAdam or FusedSGD: the guard runs inside their step()")
        guard = optimizer.guard = GradGuard(max_norm=clip_grad_norm, skip_nonfinite=skip_nonfinite)
    if ema is None:
        ema = getattr(optimizer, "ema", None)
    if ema is None and ema_decay > 0:
        from ..optim import WeightEMA, _FlatOptimizer
        if not isinstance(optimizer, _FlatOptimizer):
            raise TypeError("ema_decay needs a FusedAdam or FusedSGD: the average is updated inside their step()")
        ema = WeightEMA(model, decay=ema_decay, warmup=ema_warmup)
        optimizer._take_ema(ema)
    ema_by_hand = ema is not None and getattr(optimizer, "ema", None) is not ema      # a torch optimizer: the loop updates the average itself
    best_val_loss = float('inf')
    best_epoch = 0
    max_tolerance = 8
    tolerance = 0
    device = next(model.parameters()).device

    def on_row(k, row, meta):
        if progress is not None:
            geo = row[1] if meta is None else meta               # meta: a geo loss that lives on the host (the int 0 without include_geo)
            progress(format_batch_description(k, row[0], geo, row[2]))

    slog = trainlog.StepLog(3, ring=ring, device=device, on_row=on_row)
    for epoch in range(epochs):
        log(f"EPOCH {epoch}")
        model.train()
        host_sum = 0                                             # total_loss[1] of the steps whose geo loss lives on the host
        any_device_geo = False
        if epoch:
            slog.reset()
        try:
            for x_batch, y_hm_batch, y_points_batch, image_name, _ in trainlog.device_batches(dataloader, device):
                slog.drain()
                # Zero the gradients.
                if optimizer is not None:
                    optimizer.zero_grad()
                # Compute output and loss.
                output = model(x_batch)
                loc_loss, geo_loss, loss = loss_function(output[0], output[1], y_hm_batch, y_points_batch)
                loss.backward()
                optimizer.step()
                if ema_by_hand:
                    ema.update()
                if torch.is_tensor(geo_loss) and geo_loss.is_cuda:
                    any_device_geo = True
                    slog.record([loc_loss, geo_loss, loss], None, meta=None)
                else:
                    g = _host_number(geo_loss)
                    host_sum += g
                    slog.record([loc_loss, None, loss], None, meta=g)
        except BaseException:
            try:
                slog.drain()
            except Exception:
                pass
            raise
        slog.drain(block=True)
        batch_num = slog.steps
        sums = slog.sums()
        if stats is not None:
            stats.setdefault("host_waits", []).append(slog.host_waits - sum(stats.get("host_waits", [])))
        # total_loss[1]: the device's sum when the geo loss is a device tensor; the host's `0 + 0 + ...` (an int) when it never was
        total_loss = [sums[0], sums[1] + host_sum if any_device_geo else host_sum, sums[2]]
        log(format_epoch_line(total_loss, batch_num))
        if guard is not None:
            log(guard.summary_line("train", epoch))
        if kptaug is not None:
            log(kptaug.summary_line("train", epoch))
        with (ema.applied() if ema is not None else contextlib.nullcontext()):
            val_loc_loss, val_geo_loss, val_loss = eval_model(model=model, dataloader=val_dataloader, loss_function=loss_function,
                                                              input_size=input_size)

        # Position suggested by https://pytorch.org/docs/stable/optim.html#how-to-adjust-learning-rate
        scheduler.step()

        if val_loss < best_val_loss:
            best_val_loss = val_loss
            best_epoch = epoch
            tolerance = 0
            if save_checkpoints:
                log(f"ONNX export is not part of this build: no best_keypoints_{input_size[0]}{input_size[1]}.onnx written for epoch {epoch}")
        else:
            tolerance += 1

        if save_checkpoints and epoch != 0 and (epoch + 1) % intervals == 0:
            # Save the latest weights
            gs_pt_uri = os.path.join(output_uri, "{epoch}_loss_{loss}.pt".format(epoch=epoch, loss=round(val_loss, 2)))
            log(f'Saving model to {gs_pt_uri}')
            checkpoint = {'epoch': epoch,
                          'model': model.state_dict(),
                          'optimizer': optimizer.state_dict()}
            if ema is not None:
                checkpoint['ema'] = ema.state_dict()
            torch.save(checkpoint, gs_pt_uri)
        if tolerance >= max_tolerance:
            log(f"Training is stopped due; loss no longer decreases. Epoch {best_epoch} is has the best validation loss.")
            break
