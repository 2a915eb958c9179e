"""-m gpu: the native training loops (mdcv.yolo.train.run_epoch / train, mdcv.rektnet.train.train_model) against the reference's loop
statements, restated here in the manner of tests/helpers/train_loop_stub.py and run on the same drop-in classes, optimizer, weights and
batches: printed lines equal as strings, sums `==`, parameters `torch.equal`.  Mini fixtures, batches of 2-4 images, 6 steps."""
import contextlib
import io
import os
import shutil
import time
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mdcv import trainlog  # noqa: E402
from mdcv.optim import FusedAdam  # noqa: E402
from mdcv.rektnet import eval_model  # noqa: E402
from mdcv.rektnet.cross_ratio_loss import CrossRatioLoss  # noqa: E402
from mdcv.rektnet.keypoint_net import KeypointNet  # noqa: E402
from mdcv.rektnet.train import train_model  # noqa: E402
from mdcv.yolo.models import Darknet  # noqa: E402
from mdcv.yolo.train import run_epoch, train  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MINI = os.path.join(G, "mini")
device = torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------ the reference's statements
def reference_run_epoch(label_prefix, data_loader, num_steps, optimizer, model, epoch, num_epochs, step):
    """CVC-YOLOv3/train.py:49-93"""
    print(f"Model in {label_prefix} mode")
    epoch_losses = [0.0] * 7
    epoch_time_total = 0.0
    epoch_num_targets = 1e-12
    t1 = time.time()
    loss_labels = ["Total", "L-x", "L-y", "L-w", "L-h", "L-noobj", "L-obj"]
    for i, (img_uri, imgs, targets) in enumerate(data_loader):
        if step[0] >= num_steps:
            break
        imgs = imgs.to(device, non_blocking=True)
        targets = targets.to(device, non_blocking=True)
        targets.requires_grad_(False)
        step_num_targets = ((targets[:, :, 1:5] > 0).sum(dim=2) > 1).sum().item() + 1e-12
        epoch_num_targets += step_num_targets
        if optimizer is not None:
            optimizer.zero_grad()
        losses = model(imgs, targets)
        if label_prefix == "train":
            losses[0].sum().backward()
        if optimizer is not None:
            optimizer.step()
        for j, (label, loss) in enumerate(zip(loss_labels, losses)):
            batch_loss = loss.sum().to('cpu').item()
            epoch_losses[j] += batch_loss
        finished_time = time.time()
        step_time_total = finished_time - t1
        epoch_time_total += step_time_total
        statement = label_prefix + ' Epoch: ' + str(epoch) + ', Batch: ' + str(i + 1) + '/' + str(len(data_loader))
        count = 0
        for (loss_label, loss) in zip(loss_labels, losses):
            if count == 0:
                statement += ', Total: ' + '{0:10.6f}'.format(loss.item() / step_num_targets)
                tot_loss = loss.item()
                count += 1
            else:
                statement += ',   ' + loss_label + ': {0:5.2f}'.format(loss.item() / tot_loss * 100) + '%'
        print(statement)
        if label_prefix == "train":
            step[0] += 1
    return epoch_losses, epoch_time_total, epoch_num_targets


class _Bar:
    """what the statements below need of tqdm: iteration and set_description"""

    def __init__(self, it, sink):
        self.it, self.sink = it, sink

    def __iter__(self):
        return iter(self.it)

    def set_description(self, text):
        self.sink.append(text)


def reference_train_epochs(model, dataloader, loss_function, optimizer, scheduler, epochs, val_dataloader, input_size, descriptions):
    """RektNet/train_eval.py:52-85 (the ONNX / checkpoint / tolerance tail is host bookkeeping on val_loss and is not restated)"""
    for epoch in range(epochs):
        print(f"EPOCH {epoch}")
        model.train()
        total_loss = [0, 0, 0]
        batch_num = 0
        train_process = _Bar(dataloader, descriptions)
        for x_batch, y_hm_batch, y_points_batch, image_name, _ in train_process:
            x_batch = x_batch.to(device)
            y_hm_batch = y_hm_batch.to(device)
            y_points_batch = y_points_batch.to(device)
            if optimizer is not None:
                optimizer.zero_grad()
            output = model(x_batch)
            loc_loss, geo_loss, loss = loss_function(output[0], output[1], y_hm_batch, y_points_batch)
            loss.backward()
            optimizer.step()
            loc_loss, geo_loss, loss = loc_loss.item(), geo_loss.item(), loss.item()
            train_process.set_description(f"Batch {batch_num}. Location Loss: {round(loc_loss,5)}. Geo Loss: {round(geo_loss,5)}. Total Loss: {round(loss,5)}")
            total_loss[0] += loc_loss
            total_loss[1] += geo_loss
            total_loss[2] += loss
            batch_num += 1
        print(f"\tTraining: MSE/Geometric/Total Loss: {round(total_loss[0]/batch_num,10)}/{round(total_loss[1]/batch_num,10)}/{round(total_loss[2]/batch_num,10)}")
        eval_model(model=model, dataloader=val_dataloader, loss_function=loss_function, input_size=input_size)
        scheduler.step()


# ------------------------------------------------------------------------------------------------------------ fixtures
def new_darknet():
    cwd = os.getcwd()
    os.chdir(MINI)
    try:
        net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False)
        net.load_weights("mini.weights", net.get_start_weight_dim())
    finally:
        os.chdir(cwd)
    return net.to(device).train()


def yolo_batches(n, B=2, T=4, seed=5, where="cuda"):
    """a fixed list of (uris, imgs, targets): random images, 1..T boxes per image with centres inside the frame, zero padding rows"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(n):
        x = torch.rand(B, 3, 64, 64, generator=g)
        t = torch.zeros(B, T, 5)
        for b in range(B):
            m = 1 + (k + b) % T
            t[b, :m, 1:3] = 0.1 + 0.8 * torch.rand(m, 2, generator=g)
            t[b, :m, 3:5] = 0.05 + 0.3 * torch.rand(m, 2, generator=g)
        if where == "cuda":
            x, t = x.cuda(), t.cuda()
        elif where == "pinned":
            x, t = x.pin_memory(), t.pin_memory()
        out.append(([f"img{k}_{b}" for b in range(B)], x, t))
    return out


def flat(model):
    return model.flat_parameters()[0].clone()


def captured(fn, *a, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ret = fn(*a, **kw)
    return buf.getvalue().splitlines(), ret


_REF = {}


def yolo_reference(mode, num_steps):
    """the reference's statements over the fixed batches, once per case: (lines, epoch_losses, epoch_num_targets, step, parameters)"""
    key = (mode, num_steps)
    if key not in _REF:
        net = new_darknet()
        step = [0]
        if mode == "train":
            lines, ret = captured(reference_run_epoch, "train", yolo_batches(6), num_steps, FusedAdam(net, lr=1e-3), net, 3, 9, step)
        else:
            with torch.no_grad():
                lines, ret = captured(reference_run_epoch, "validate", yolo_batches(6), num_steps, None, net, 3, 9, step)
        _REF[key] = (lines, ret[0], ret[2], step[0], flat(net))
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------ YOLO
@pytest.mark.parametrize("mode,num_steps", [("train", 100), ("validate", 100), ("train", 4)])
def test_run_epoch_prints_sums_and_updates_what_the_reference_loop_does(mode, num_steps):
    want_lines, want_losses, want_targets, want_step, want_params = yolo_reference(mode, num_steps)
    assert len(want_lines) == 1 + min(6, num_steps)
    net = new_darknet()
    step, lines = [0], []
    if mode == "train":
        ret = run_epoch("train", yolo_batches(6), num_steps, FusedAdam(net, lr=1e-3), net, 3, 9, step, log=lines.append)
    else:
        with torch.no_grad():
            ret = run_epoch("validate", yolo_batches(6), num_steps, None, net, 3, 9, step, log=lines.append)
    assert lines == want_lines
    assert ret[0] == want_losses and ret[2] == want_targets
    assert isinstance(ret[0], list) and len(ret[0]) == 7 and all(isinstance(v, float) for v in ret[0]) and ret[1] > 0
    assert step[0] == want_step == (0 if mode == "validate" else min(6, num_steps))
    assert torch.equal(flat(net), want_params)


def test_ring_wrap_keeps_every_line_in_order():
    runs = {}
    for ring in (64, 2):
        net = new_darknet()
        lines, stats = [], {}
        run_epoch("train", yolo_batches(7), 100, FusedAdam(net, lr=1e-3), net, 1, 1, [0], log=lines.append, ring=ring, stats=stats)
        runs[ring] = (lines, stats, flat(net))
    assert len(runs[2][0]) == 8 and [l.split(",")[1] for l in runs[2][0][1:]] == [f" Batch: {k}/7" for k in range(1, 8)]
    assert runs[2][0] == runs[64][0] and torch.equal(runs[2][2], runs[64][2])
    assert runs[64][1] == {"host_waits": 1, "steps": 7}
    assert runs[2][1]["steps"] == 7 and 1 <= runs[2][1]["host_waits"] <= 6      # the end, and at most one per step behind the second


def test_host_batches_through_prefetch_give_the_same_epoch():
    want_lines, want_losses, want_targets, _, want_params = yolo_reference("train", 100)
    for where in ("pinned", "cpu"):
        net = new_darknet()
        lines = []
        ret = run_epoch("train", yolo_batches(6, where=where), 100, FusedAdam(net, lr=1e-3), net, 3, 9, [0], log=lines.append)
        assert lines == want_lines and ret[0] == want_losses and ret[2] == want_targets
        assert torch.equal(flat(net), want_params)
    moved = list(trainlog.prefetch(yolo_batches(3, where="pinned"), device))
    assert all(x.is_cuda and t.is_cuda and isinstance(u, list) for u, x, t in moved)
    assert all(torch.equal(x.cpu(), h[1]) and torch.equal(t.cpu(), h[2]) for (u, x, t), h in zip(moved, yolo_batches(3, where="cpu")))
    assert list(trainlog.prefetch([], device)) == []


def test_the_native_steps_make_no_blocking_read():
    net = new_darknet()
    opt = FusedAdam(net, lr=1e-3)
    batches = yolo_batches(6)
    run_epoch("train", batches, 100, opt, net, 1, 2, [0], log=lambda line: None)       # plans, flat buffers, optimizer state: built
    probe = torch.ones(1, device=device)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as control:
            warnings.simplefilter("always")
            probe.item()                                                               # the positive control: one blocking read
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            lines = []
            run_epoch("train", batches, 100, opt, net, 2, 2, [0], log=lines.append)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(lines) == 7
    if not any("synchroniz" in str(w.message).lower() for w in control):
        pytest.skip("torch.cuda.set_sync_debug_mode('warn') does not warn on .item() in this torch build: nothing to assert")
    assert [str(w.message) for w in seen if "synchroniz" in str(w.message).lower()] == []


def test_an_exception_out_of_a_step_lets_the_landed_lines_out_first():
    net = new_darknet()
    batches = yolo_batches(4)
    bad = batches[2][2].clone()
    bad[0, 0, 1] = 1.0                                                                 # cx == 1.0: the reference's IndexError
    batches[2] = (batches[2][0], batches[2][1], bad)
    lines = []
    with pytest.raises(IndexError):
        run_epoch("train", batches, 100, FusedAdam(net, lr=1e-3), net, 1, 1, [0], log=lines.append)
    # the label is refused at the end of step 2's backward: steps 0 and 1 were recorded, and those of their lines that had landed came out
    assert lines[0] == "Model in train mode" and len(lines) <= 3
    assert all(l.startswith(f"train Epoch: 1, Batch: {k}/4, Total:") for k, l in enumerate(lines[1:], 1))


# ------------------------------------------------------------------------------------------------------------ RektNet
def new_keypoint_net():
    zs = np.load(os.path.join(G, "rektnet_net.npz"))
    model = KeypointNet(7, (80, 80))
    model.load_state_dict({k[4:]: torch.from_numpy(zs[k]) for k in zs.files if k.startswith("sd::")})
    return model.to(device)


def crop_batches(n, B=4, seed=9):
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(n):
        x = torch.rand(B, 3, 80, 80, generator=g)
        pts = torch.rand(B, 7, 2, generator=g) * (79 / 80)
        out.append((x.cuda(), torch.zeros(B, 7, 80, 80, device=device), pts.cuda(), [f"c{k}_{b}" for b in range(B)], [(80, 80, 3)] * B))
    return out


@pytest.mark.parametrize("include_geo", [False, True])
def test_train_model_matches_the_reference_epochs(include_geo, tmp_path):
    def setup():
        model = new_keypoint_net()
        with contextlib.redirect_stdout(io.StringIO()):
            loss_function = CrossRatioLoss("l1_softargmax", include_geo, 0.05, 0.05)
        optimizer = FusedAdam(model, lr=1e-3)
        return model, loss_function, optimizer, torch.optim.lr_scheduler.ExponentialLR(optimizer, gamma=0.9)
    train_batches, val_batches = crop_batches(3), crop_batches(1, seed=10)
    model, loss_function, optimizer, scheduler = setup()
    want_desc = []
    want_lines, _ = captured(reference_train_epochs, model, train_batches, loss_function, optimizer, scheduler, 2, val_batches, (80, 80), want_desc)
    want_state = {k: v.clone() for k, v in model.state_dict().items()}

    model, loss_function, optimizer, scheduler = setup()
    desc, lines, stats = [], [], {}
    val_lines, _ = captured(train_model, model, str(tmp_path), train_batches, loss_function, optimizer, scheduler, 2, val_batches, 2, (80, 80), 7,
                            True, ["k%d" % k for k in range(7)], "study", False, progress=desc.append, log=lines.append, stats=stats)
    assert desc == want_desc and len(desc) == 6
    assert ("Geo Loss: 0. Total" in desc[0]) == (not include_geo)                     # the int 0 of the loss without its geometric part
    training = [l for l in want_lines if l.startswith("\tTraining:")]
    assert [l for l in lines if l.startswith("\tTraining:")] == training and len(training) == 2
    assert [l for l in lines if l.startswith("EPOCH")] == ["EPOCH 0", "EPOCH 1"]
    assert val_lines == [l for l in want_lines if "alidation" in l]                   # eval_model's own prints, same values
    got_state = model.state_dict()
    assert got_state.keys() == want_state.keys() and all(torch.equal(got_state[k], want_state[k]) for k in want_state)
    assert stats["host_waits"] == [1, 1]
    # the reference's interval rule: epoch != 0 and (epoch + 1) % intervals == 0 -> epoch 1 of 2 with intervals = 2
    saved = sorted(p.name for p in tmp_path.iterdir())
    assert len(saved) == 1 and saved[0].startswith("1_loss_") and saved[0].endswith(".pt")
    ck = torch.load(tmp_path / saved[0], weights_only=False)
    assert sorted(ck) == ["epoch", "model", "optimizer"] and ck["epoch"] == 1
    assert all(torch.equal(ck["model"][k].to(device), got_state[k]) for k in got_state)
    assert any("ONNX" in l for l in lines)


# ------------------------------------------------------------------------------------------------------------ train(...)
def mini_dataset(tmp_path):
    """mini.cfg / mini.weights and a dataset CSV made of the mini anchors row and the imgload frames' rows, in a fresh directory"""
    for name in ("mini.cfg", "mini.weights"):
        shutil.copy(os.path.join(MINI, name), tmp_path / name)
    os.makedirs(tmp_path / "dataset")
    anchors = open(os.path.join(MINI, "dataset", "train.csv")).readline()
    rows = open(os.path.join(G, "imgload", "dataset.csv")).read().splitlines()[1:]
    for name in ("train.csv", "validate.csv"):
        with open(tmp_path / "dataset" / name, "w") as f:
            f.write(anchors.rstrip("\n") + "\n" + "\n".join(rows) + "\n")
    z = np.load(os.path.join(G, "imgload", "frames.npz"))
    frames = {k: z[k] for k in z.files}
    return lambda p: frames[os.path.splitext(os.path.basename(p))[0]]


def train_args(**kw):
    a = dict(evaluate=False, batch_size=2, optimizer_pick="Adam", model_cfg="mini.cfg", weights_path="mini.weights", output_path="out",
             dataset_path="", num_epochs=2, num_steps=1000, checkpoint_interval=1, augment_affine=False, augment_hsv=False, lr_flip=False,
             ud_flip=False, momentum=0.9, gamma=0.95, lr=1e-3, weight_decay=0.0, vis_batch=0, data_aug=False, blur=False, salt=False,
             noise=False, contrast=False, sharpen=False, ts=False, debug_mode=False, upload_dataset=False, xy_loss=2.0, wh_loss=1.6,
             no_object_loss=25.0, object_loss=0.1, vanilla_anchor=False, val_tolerance=3, min_epochs=0, num_workers=1)
    a.update(kw)
    return a


def reference_stop(val_losses, val_tolerance, min_epochs, checkpoint_interval=1):
    """train.py:201-256's bookkeeping on the sequence of average validation losses -> (checks made, val_loss returned)"""
    val_loss, val_loss_counter = 999, 0
    for n, avg_epoch_loss in enumerate(val_losses, 1):
        epoch = n * checkpoint_interval
        if avg_epoch_loss > val_loss and epoch > min_epochs:
            val_loss_counter += 1
        else:
            val_loss_counter = 0
            val_loss = avg_epoch_loss
        if val_loss_counter == val_tolerance:
            return n, val_loss
    return len(val_losses), val_loss


def test_train_end_to_end_checkpoints_result_file(tmp_path, monkeypatch):
    decode = mini_dataset(tmp_path)
    monkeypatch.chdir(tmp_path)
    os.makedirs("out")
    lines, state = [], {}
    with contextlib.redirect_stdout(io.StringIO()):
        val_loss = train(**train_args(), decode=decode, log=lines.append, state=state)
    model = state["model"]
    assert state["epoch"] == 2 and state["step"][0] == 4                               # 4 frames (one CSV row is skipped), batches of 2
    assert sorted(os.listdir("out")) == ["1.weights", "2.weights"]
    again = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False)
    again.load_weights("out/2.weights", again.get_start_weight_dim())
    # (parameters: the BatchNorm running statistics move on after the checkpoint, in the validation-loss epoch, as in the reference)
    live = dict(model.named_parameters())
    reloaded = dict(again.named_parameters())
    assert [k for k, v in live.items() if not torch.equal(reloaded[k], v.detach().cpu())] == [] and len(live) > 30
    first = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False)
    first.load_weights("out/1.weights", first.get_start_weight_dim())
    assert any(not torch.equal(p, q) for p, q in zip(first.parameters(), again.parameters()))      # epoch 2 trained on
    printed = [l for l in lines if l.startswith("Average Validation Loss:")]
    assert len(printed) == 2 == len(state["val_losses"])
    assert reference_stop(state["val_losses"], 3, 0) == (2, val_loss)
    kept = float(open("logs/result.txt").read())
    assert kept == val_loss and 'Average Validation Loss: {0:10.6f}'.format(kept) in printed
    assert [l for l in lines if l.startswith("train Epoch: 2, Batch:")][-1].startswith("train Epoch: 2, Batch: 2/2, Total:")
    assert sum(l.startswith("validate Epoch:") for l in lines) == 4 and lines.count("Completed epoch:  2") == 1


def test_train_stops_on_val_tolerance_like_the_reference(tmp_path, monkeypatch):
    decode = mini_dataset(tmp_path)
    monkeypatch.chdir(tmp_path)
    os.makedirs("out")
    lines, state = [], {}
    with contextlib.redirect_stdout(io.StringIO()):
        val_loss = train(**train_args(lr=0.0, val_tolerance=1, num_epochs=8, ts=True), decode=decode, log=lines.append, state=state)
    # a learning rate of 0 leaves the parameters alone; with tile-and-scale the validation patches are drawn anew every epoch, so the
    # average validation loss moves, and the first rise after a check is the stop
    checks, want = reference_stop(state["val_losses"], 1, 0)
    assert len(state["val_losses"]) == checks == state["epoch"] and val_loss == want
    assert checks < 8, state["val_losses"]
    assert "Validation loss stopped decreasing over the last 1 checkpoints, creating onnx file" in lines
    assert any("no ONNX file written" in l for l in lines) and os.path.exists(os.path.join("out", state["model"].get_onnx_name()))
    assert lines.count("Validation loss did not decrease for 1 consecutive check(s)") == 1
