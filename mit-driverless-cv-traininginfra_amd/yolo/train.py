"""The native form of the reference's CVC-YOLOv3/train.py: `run_epoch` (train.py:49-93) and `train` (its `main`, train.py:95-259).

Same lines, sums, checkpoints, `logs/result.txt` and stopping rule -- but the per-step bookkeeping is one HIP launch (`mdcv.trainlog`,
csrc/train_log.hip) instead of sixteen blocking `.item()` / `.to('cpu')` reads, the optimizer is `FusedAdam` / `FusedSGD`, batches come
from `ImageLabelBatches` on the device (host batches are moved one batch ahead on a copy stream), and the loop never waits for the GPU
inside an epoch: a step's line is printed when its row has landed on the host, a few steps late.

    python -m mdcv.yolo.train --model_cfg model_cfg/yolo_baseline.cfg --weights_path sample-yolov3.weights ...

takes train.py's flags.  Not done here: the ONNX export behind the early stop (the weights are saved under the name the reference
renames them to, and a line says so), `vis_batch` drawing and `upload_dataset` (accepted and ignored, as the loader does).
"""
import argparse
import contextlib
import os
import time
from datetime import datetime

import torch

from .. import trainlog

LOSS_LABELS = ["Total", "L-x", "L-y", "L-w", "L-h", "L-noobj", "L-obj"]


def format_step_line(label_prefix, epoch, i, n_batches, row):
    """The statement train.py:81-90 prints for batch `i` (0-based) of `n_batches`, from the step's row: seven losses and the count of
    labelled targets, as Python floats.  The reference's own expressions on the same numbers: the total over `count + 1e-12`, every part
    as a percentage of the total -- so a total of 0.0 raises ZeroDivisionError and a NaN total prints nan, as there."""
    step_num_targets = row[7] + 1e-12
    tot_loss = row[0]
    statement = label_prefix + ' Epoch: ' + str(epoch) + ', Batch: ' + str(i + 1) + '/' + str(n_batches)
    statement += ', Total: ' + '{0:10.6f}'.format(tot_loss / step_num_targets)
    for loss_label, loss in zip(LOSS_LABELS[1:], row[1:7]):
        statement += ',   ' + loss_label + ': {0:5.2f}'.format(loss / tot_loss * 100) + '%'
    return statement


def run_epoch(label_prefix, data_loader, num_steps, optimizer, model, epoch, num_epochs, step, log=print, ring=64, stats=None, guard=None):
    """train.py:49-93 with the reference's signature and return value `(epoch_losses, epoch_time_total, epoch_num_targets)`:
    `epoch_losses[j]` is the float sum of the steps' loss j and `epoch_num_targets` is `1e-12 + sum(count + 1e-12)`, both added on the
    device in the reference's order (bit for bit the reference's Python sums).  The `num_steps` break, `step[0] += 1` in "train" mode
    only and `optimizer=None` (the validation-loss epoch, which the caller wraps in `torch.no_grad()`) are the reference's.

    `log(line)` gets "Model in ... mode" and then one line per step, each equal to the reference's, late but complete and in order; all
    of them have been handed over when this returns or raises.  An exception out of a step (the model's IndexError for a label with
    cx / cy >= 1.0, say) lets the lines that have landed out first.

    `epoch_time_total` is the epoch's wall time.  The reference's value adds up, per step, the time since the epoch's START
    (train.py:77-79), which grows quadratically with the number of steps and measures nothing; it is not reproduced.

    Batches that are already on the device are consumed as they are; host batches go through `trainlog.prefetch`.  The loop itself
    never waits for the GPU: `StepLog.host_waits` is 1 (the epoch's end) unless more than `ring` steps are in flight; a `stats` dict
    receives `host_waits` and `steps`.  (The model's own look at its bad-label flag behind each backward is unchanged;
    `model.strict_targets = False` makes that a query too.)

    `guard`: the `mdcv.optim.GradGuard` to report on; default: the one the optimizer holds (the optimizer, not this loop, runs it).  With a
    guard, ONE more line follows the reference's lines, after the epoch's wait and from one read of the guard's counters:
    `train Epoch: 3, grad norm max 41.2 mean 7.9, clipped 12, skipped 1 of 240 steps`.  Without a guard there is no such line and
    no such read."""
    if guard is None and optimizer is not None:
        guard = getattr(optimizer, "guard", None)
    log(f"Model in {label_prefix} mode")
    device = next(model.parameters()).device
    n_batches = len(data_loader)
    slog = trainlog.StepLog(7, ring=ring, device=device,
                            on_row=lambda k, row, i: log(format_step_line(label_prefix, epoch, i, n_batches, row)))
    t1 = time.time()
    try:
        for i, (img_uri, imgs, targets) in enumerate(trainlog.device_batches(data_loader, device)):
            if step[0] >= num_steps:
                break
            slog.drain()
            targets.requires_grad_(False)
            # Compute loss, compute gradient, update parameters
            if optimizer is not None:
                optimizer.zero_grad()
            losses = model(imgs, targets)
            if label_prefix == "train":
                losses[0].sum().backward()
            if optimizer is not None:
                optimizer.step()
            slog.record([loss if loss.dim() == 0 else loss.sum() for loss in losses], targets, meta=i)
            if label_prefix == "train":
                step[0] += 1
    except BaseException:
        try:
            slog.drain()                                         # what has landed; no wait behind a failed step
        except Exception:
            pass
        raise
    slog.drain(block=True)
    sums = slog.sums()
    if guard is not None:
        log(guard.summary_line(label_prefix, epoch))
    if stats is not None:
        stats["host_waits"], stats["steps"] = slog.host_waits, slog.steps
    return sums[:7], time.time() - t1, sums[7]


def _output_uri(output_path, model_cfg):
    if output_path != "automatic":
        return output_path
    current_month = datetime.now().strftime('%B').lower()
    current_year = str(datetime.now().year)
    uri = os.path.join('outputs/', current_month + '-' + current_year + '-experiments/' + model_cfg.split('.')[0].split('/')[-1])
    os.makedirs(uri, exist_ok=True)
    return uri


def train(*, evaluate, batch_size, optimizer_pick, model_cfg, weights_path, output_path, dataset_path, num_epochs, num_steps,
          checkpoint_interval, augment_affine, augment_hsv, lr_flip, ud_flip, momentum, gamma, lr, weight_decay, vis_batch, data_aug, blur,
          salt, noise, contrast, sharpen, ts, debug_mode, upload_dataset, xy_loss, wh_loss, no_object_loss, object_loss, vanilla_anchor,
          val_tolerance, min_epochs, log=print, device=None, precision=None, decode=None, num_workers=None, cache_bytes=None, state=None,
          clip_grad_norm=0.0, skip_nonfinite=False, ema_decay=0.0, ema_warmup=10, mosaic=0.0, mosaic_off_epochs=0):
    """train.py's `main` (train.py:95-259) with its keyword arguments, on the native pieces: `ImageLabelBatches` for both loaders (the
    reference's option mapping: the validation loader without augmentation, flips or shuffling; batch size 1 and no shuffle in
    `debug_mode`), `FusedAdam` / `FusedSGD`, `StepLR(step_size=1, gamma)` stepped at the top of every epoch as there, `run_epoch` above,
    a `<epoch>.weights` checkpoint every `checkpoint_interval` epochs (and at the last epoch / step), the validation-loss epoch under
    `no_grad`, `logs/result.txt`, the `val_tolerance` / `min_epochs` stop, `validate(...)` for mAP, and `evaluate=True`.  Returns `val_loss`.

    Beyond the reference's arguments: `log` (every line goes through it), `device`, `precision` (Darknet's), and the loaders' `decode`,
    `num_workers`, `cache_bytes`; `state`, a dict, receives the live `model`, `optimizer`, `epoch`, `step` and `val_losses` (the average
    validation loss of every check, in order) for a caller that wants more than the return value.  The ONNX export is not done: on the early stop the weights are saved as `<output>/<onnx_name>`, the
    file the reference leaves there, and a line says that no ONNX file was written.

    `clip_grad_norm` > 0 and / or `skip_nonfinite` attach a `GradGuard` to the optimizer (global-norm clipping, dropping a step whose
    gradient is not finite): each training epoch then logs one more line.  Both off (the default): no guard, nothing changes.

    `ema_decay` > 0 attaches a `WeightEMA(model, ema_decay, ema_warmup)` to the optimizer.  The checkpoint block then runs
    with the averaged weights and BatchNorm statistics swapped in: `<epoch>.weights`, the validation-loss epoch, `logs/result.txt`, the
    stopping rule, `validate(...)` and the early stop's `<onnx_name>` file describe the averaged model; the live weights go to
    `<epoch>.live.weights` (what a continued run loads), and one more line per checkpoint states the update count and the current decay
    (one host read).  `evaluate=True` validates the weights it loaded.  0 (the default): no EMA, nothing changes.

    `mosaic` > 0 wraps the TRAINING loader in `MosaicBatches(p=mosaic)`: each training image is, with that probability,
    composed from four tiles of its batch on the device.  The validation loader never is.  The last `mosaic_off_epochs` epochs of
    `num_epochs` run on the loader's own batches.  One more line follows each training epoch, after the epoch's wait and from one read of the
    wrapper's counters.  0 (the default): no wrapper is constructed, nothing changes."""
    from .models import Darknet
    from .validate import validate
    from ..data.images import ImageLabelBatches
    from ..data.mosaic import MosaicBatches
    from ..optim import FusedAdam, FusedSGD, GradGuard, WeightEMA
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)

    log("Initializing model")
    model = Darknet(config_path=model_cfg, xy_loss=xy_loss, wh_loss=wh_loss, no_object_loss=no_object_loss, object_loss=object_loss,
                    vanilla_anchor=vanilla_anchor, precision=precision)
    img_width, img_height = model.img_size()
    bw = model.get_bw()
    validate_uri, train_uri = model.get_links()
    output_uri = _output_uri(output_path, model_cfg)
    num_validate_images, num_train_images = model.num_images()
    conf_thresh, nms_thresh, iou_thresh = model.get_threshs()
    onnx_name = model.get_onnx_name()

    log("Initializing data loaders")
    extra = dict(device=device, decode=decode, num_workers=num_workers, cache_bytes=cache_bytes, vis_batch=vis_batch,
                 upload_dataset=upload_dataset, debug_mode=debug_mode, ts=ts, bw=bw, batch_size=(1 if debug_mode else batch_size))
    train_data_loader = ImageLabelBatches(train_uri, dataset_path, img_width, img_height, num_images=num_train_images,
                                          augment_hsv=augment_hsv, augment_affine=augment_affine, lr_flip=lr_flip, ud_flip=ud_flip,
                                          data_aug=data_aug, blur=blur, salt=salt, noise=noise, contrast=contrast, sharpen=sharpen,
                                          shuffle=(False if debug_mode else True), **extra)
    if mosaic > 0:
        train_data_loader = MosaicBatches(train_data_loader, p=mosaic)
    log("Num train images:  " + str(len(train_data_loader.dataset)))
    validate_data_loader = ImageLabelBatches(validate_uri, dataset_path, img_width, img_height, num_images=num_validate_images,
                                             augment_hsv=False, augment_affine=False, lr_flip=False, ud_flip=False, data_aug=False,
                                             blur=False, salt=False, noise=False, contrast=False, sharpen=False, shuffle=False, **extra)
    log("Num validate images:  " + str(len(validate_data_loader.dataset)))

    log("Training batch size: " + str(batch_size))
    log("Checkpoint interval: " + str(checkpoint_interval))
    log("Loss constants: " + str(model.get_loss_constant()))
    log("Anchor boxes: " + str(model.get_anchors()))
    log("Training image width: " + str(img_width))
    log("Training image height: " + str(img_height))
    log("Confidence Threshold: " + str(conf_thresh))
    log("Number of training classes: " + str(model.get_num_classes()))
    log("Conv activation type: " + str(model.get_conv_activation()))
    log("Starting learning rate: " + str(lr))
    log("Tile and scale mode [on]" if ts else "Tile and scale mode [off]")
    log("Data augmentation mode [on]" if data_aug else "Data augmentation mode [off]")

    log("Loading weights")
    model.load_weights(weights_path, model.get_start_weight_dim())
    model = model.to(device, non_blocking=True)
    guard = GradGuard(max_norm=clip_grad_norm, skip_nonfinite=skip_nonfinite) if clip_grad_norm > 0 or skip_nonfinite else None
    ema = WeightEMA(model, decay=ema_decay, warmup=ema_warmup) if ema_decay > 0 else None
    more = {} if ema is None else {"ema": ema}
    if optimizer_pick == "Adam":
        log("Using Adam Optimizer")
        optimizer = FusedAdam(model, lr=lr, weight_decay=weight_decay, guard=guard, **more)
    elif optimizer_pick == "SGD":
        log("Using SGD Optimizer")
        optimizer = FusedSGD(model, lr=lr, momentum=momentum, weight_decay=weight_decay, guard=guard, **more)
    else:
        raise Exception(f"Invalid optimizer name: {optimizer_pick}")
    scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=1, gamma=gamma)

    val_loss = 999  # using a high number for validation loss
    val_loss_counter = 0
    step = [0]  # wrapping in an array so it is mutable
    epoch = 0
    state = {} if state is None else state
    state.update(model=model, optimizer=optimizer, epoch=0, step=step, val_losses=[])
    try:
        while epoch < num_epochs and step[0] < num_steps and not evaluate:
            epoch += 1
            state["epoch"] = epoch
            scheduler.step()
            model.train()
            if mosaic > 0:
                train_data_loader.active = epoch <= num_epochs - mosaic_off_epochs
            run_epoch(label_prefix="train", data_loader=train_data_loader, epoch=epoch, step=step, model=model, num_epochs=num_epochs,
                      num_steps=num_steps, optimizer=optimizer, log=log)
            if mosaic > 0:
                log(train_data_loader.summary_line("train", epoch))
            log('Completed epoch:  ' + str(epoch))
            if epoch % checkpoint_interval == 0 or epoch == num_epochs or step[0] >= num_steps:
                if ema is not None:
                    model.save_weights(os.path.join(output_uri, "{epoch}.live.weights".format(epoch=epoch)))
                    log(ema.summary_line("train", epoch))
                stop = False
                with (ema.applied() if ema is not None else contextlib.nullcontext()):      # the averaged model, from here to the end of the block
                    model.save_weights(os.path.join(output_uri, "{epoch}.weights".format(epoch=epoch)))
                    with torch.no_grad():
                        log("Calculating loss on validate data")
                        epoch_losses, epoch_time_total, epoch_num_targets = run_epoch(
                            label_prefix="validate", data_loader=validate_data_loader, epoch=epoch, model=model, num_epochs=num_epochs,
                            num_steps=num_steps, optimizer=None, step=step, log=log)
                        avg_epoch_loss = epoch_losses[0] / epoch_num_targets
                        state["val_losses"].append(avg_epoch_loss)
                        log('Average Validation Loss: {0:10.6f}'.format(avg_epoch_loss))
                        if avg_epoch_loss > val_loss and epoch > min_epochs:
                            val_loss_counter += 1
                            log(f"Validation loss did not decrease for {val_loss_counter} consecutive check(s)")
                        else:
                            log("Validation loss decreased. Yay!!")
                            val_loss_counter = 0
                            val_loss = avg_epoch_loss
                            os.makedirs("logs", exist_ok=True)
                            with open("logs/result.txt", "w") as result:
                                result.write(str(avg_epoch_loss))
                        validate(dataloader=validate_data_loader, model=model, device=device, step=step[0], bbox_all=False,
                                 debug_mode=debug_mode)
                        if val_loss_counter == val_tolerance:
                            log("Validation loss stopped decreasing over the last " + str(val_tolerance) + " checkpoints, creating onnx file")
                            save_weights_uri = os.path.join(output_uri, onnx_name)
                            model.save_weights(save_weights_uri)
                            log(f"ONNX export is not part of this build: darknet weights saved to {save_weights_uri}, no ONNX file written")
                            stop = True
                if stop:
                    break
        if evaluate:
            validate(dataloader=validate_data_loader, model=model, device=device, step=-1, bbox_all=False, debug_mode=debug_mode)
    finally:
        train_data_loader.close()
        validate_data_loader.close()
    return val_loss


def _parser():
    parser = argparse.ArgumentParser(description="CVC-YOLOv3 training on the native loop (the flags of the reference's train.py)")

    def add_bool_arg(name, default, help):
        group = parser.add_mutually_exclusive_group(required=False)
        group.add_argument('--' + name, dest=name, action='store_true', help=help)
        group.add_argument('--no_' + name, dest=name, action='store_false', help="Do not " + help)
        parser.set_defaults(**{name: default})

    parser.add_argument('--batch_size', type=int, default=7, help='size of each image batch')
    parser.add_argument('--optimizer_pick', type=str, default="Adam", help='Adam or SGD')
    parser.add_argument('--model_cfg', type=str, required=True, help='cfg file path')
    parser.add_argument('--weights_path', type=str, default="sample-yolov3.weights", help='initial weights path')
    parser.add_argument('--output_path', type=str, default="automatic", help='output weights path; automatic: outputs/<month>-<year>-experiments/<cfg name>')
    parser.add_argument('--dataset_path', type=str, default="dataset/YOLO_Dataset/", help='path to image dataset')
    parser.add_argument('--num_epochs', type=int, default=2048, help='maximum number of epochs')
    parser.add_argument('--num_steps', type=int, default=8388608, help='maximum number of steps')
    parser.add_argument('--val_tolerance', type=int, default=3, help='tolerance for validation loss decreasing')
    parser.add_argument('--min_epochs', type=int, default=3, help='minimum training epochs')
    parser.add_argument('--checkpoint_interval', type=int, default=1, help='interval between saving model weights')
    parser.add_argument('--vis_batch', type=int, default=0, help='accepted; batches are not drawn (a non-zero value still caps the number of steps)')
    add_bool_arg('ts', True, 'scale by the cone pixel size, then chop and tile (instead of pad and resize)')
    add_bool_arg('augment_affine', False, 'augment images')
    add_bool_arg('augment_hsv', False, 'augment hsv')
    add_bool_arg('augment_lr_flip', False, 'flip left/right')
    add_bool_arg('augment_ud_flip', False, 'flip up/down')
    add_bool_arg('augment_blur', False, 'add blur')
    add_bool_arg('augment_salt', False, 'add salt/pepper')
    add_bool_arg('augment_noise', False, 'add noise')
    add_bool_arg('augment_contrast', False, 'add contrast')
    add_bool_arg('augment_sharpen', False, 'add sharpen')
    add_bool_arg('evaluate', False, 'get the mAP values rather than train')
    add_bool_arg('vanilla_anchor', False, 'use vanilla anchor boxes for training')
    add_bool_arg('debug_mode', False, 'batch size 1, no shuffle, patch 0')
    add_bool_arg('data_aug', False, 'do all stable data augmentation')
    add_bool_arg('upload_dataset', False, 'accepted and ignored')
    parser.add_argument('--momentum', type=float, default=0.9, help='momentum for the optimizer')
    parser.add_argument('--gamma', type=float, default=0.95, help='gamma for the scheduler')
    parser.add_argument('--lr', type=float, default=0.001, help='starting learning rate')
    parser.add_argument('--weight_decay', type=float, default=0.0, help='weight decay')
    parser.add_argument('--xy_loss', type=float, default=2, help='confidence loss for x and y')
    parser.add_argument('--wh_loss', type=float, default=1.6, help='confidence loss for width and height')
    parser.add_argument('--no_object_loss', type=float, default=25, help='confidence loss for non-objectness')
    parser.add_argument('--object_loss', type=float, default=0.1, help='confidence loss for objectness')
    parser.add_argument('--clip_grad_norm', type=float, default=0.0, help='clip the global gradient norm to this on the device (0 = off)')
    add_bool_arg('skip_nonfinite', False, 'drop an optimizer step whose gradient holds a NaN or an Inf, decided on the device')
    parser.add_argument('--ema_decay', type=float, default=0.0, help='validate and checkpoint an exponential moving average of the weights with this decay (0 = off)')
    parser.add_argument('--ema_warmup', type=int, default=10, help='EMA warm-up: update t uses min(ema_decay, (1 + t) / (ema_warmup + t))')
    parser.add_argument('--mosaic', type=float, default=0.0, help='compose each training image from four tiles of its batch with this probability, on the device (0 = off)')
    parser.add_argument('--mosaic_off_epochs', type=int, default=0, help='train the last N of num_epochs epochs without mosaic')
    return parser


def main(argv=None):
    opt = _parser().parse_args(argv)
    return train(evaluate=opt.evaluate, batch_size=opt.batch_size, optimizer_pick=opt.optimizer_pick, model_cfg=opt.model_cfg,
                 weights_path=opt.weights_path, output_path=opt.output_path, dataset_path=opt.dataset_path, num_epochs=opt.num_epochs,
                 num_steps=(opt.num_steps if opt.vis_batch == 0 else opt.vis_batch), checkpoint_interval=opt.checkpoint_interval,
                 augment_affine=opt.augment_affine, augment_hsv=opt.augment_hsv, lr_flip=opt.augment_lr_flip, ud_flip=opt.augment_ud_flip,
                 momentum=opt.momentum, gamma=opt.gamma, lr=opt.lr, weight_decay=opt.weight_decay, vis_batch=opt.vis_batch,
                 data_aug=opt.data_aug, blur=opt.augment_blur, salt=opt.augment_salt, noise=opt.augment_noise, contrast=opt.augment_contrast,
                 sharpen=opt.augment_sharpen, ts=opt.ts, debug_mode=opt.debug_mode, upload_dataset=opt.upload_dataset, xy_loss=opt.xy_loss,
                 wh_loss=opt.wh_loss, no_object_loss=opt.no_object_loss, object_loss=opt.object_loss, vanilla_anchor=opt.vanilla_anchor,
                 val_tolerance=opt.val_tolerance, min_epochs=opt.min_epochs, clip_grad_norm=opt.clip_grad_norm,
                 skip_nonfinite=opt.skip_nonfinite, ema_decay=opt.ema_decay, ema_warmup=opt.ema_warmup, mosaic=opt.mosaic,
                 mosaic_off_epochs=opt.mosaic_off_epochs)


if __name__ == '__main__':
    main()
