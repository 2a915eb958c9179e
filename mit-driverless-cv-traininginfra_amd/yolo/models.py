"""MI355X-native drop-in for the reference's CVC-YOLOv3/models.py (Darknet, YOLOLayer, create_modules).

Same Python surface — `Darknet(config_path, xy_loss, wh_loss, no_object_loss, object_loss, vanilla_anchor)`, the getters,
`forward(x, targets=None)`, darknet `.weights` load/save, `module_list` / `module_defs` / `hyperparams`, state_dict keys
(`module_list.<i>.conv_<i>.weight` ...) — so the reference's train.py / validate.py / detect.py call sequence runs
unchanged (reference: CVC-YOLOv3/models.py:15-422; callers train.py:100-120,182,191,196,208,217).

Underneath, `forward` does not run the nn.Modules: the cfg is lowered once per input shape into a static launch plan
(engine.Plan) of hand-written gfx950 kernels from libmdcv_hip.so — NHWC bf16 (or fp32 parity mode) implicit-GEMM MFMA
convolutions with BatchNorm statistics in the epilogue, fused BN-apply+LeakyReLU(+shortcut), zero-copy route concat,
fused YOLO heads — and the whole backward is one autograd node that runs the mirrored plan.  The nn.Modules only hold the
fp32 master parameters (OIHW) and BatchNorm buffers.  There is no CPU fallback.

Extra (non-reference) knobs: `precision=` ctor kwarg or env MDCV_PRECISION in {"bf16" (default), "fp32"};
env MDCV_GRAPH=1 replays the plan through hipGraphs.
"""
from __future__ import division

import csv
import os
from datetime import datetime

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ..engine import pad8, parse_precision
from .. import netplan
from . import lower
from .utils.parse_config import parse_model_config

vanilla_anchor_list = [[10, 13], [16, 30], [33, 23], [30, 61], [62, 45], [59, 119], [116, 90], [156, 198], [373, 326]]


def _read_anchor_row(csv_uri):
    """Row 0 of train.csv holds the k-means anchors as one quoted field 'w,h|w,h|...' (reference models.py:29-35)."""
    with open(csv_uri) as fh:
        first = next(csv.reader(fh))
    text = str(first)[2:-2]
    return [[float(v) for v in pair.split(",")] for pair in text.split("'")[0].split("|")]


class EmptyLayer(nn.Module):
    """Placeholder module for 'route' and 'shortcut' sections (keeps module_list indices aligned with the cfg)."""


def create_modules(module_defs, xy_loss, wh_loss, no_object_loss, object_loss, vanilla_anchor):
    """cfg sections -> (hyperparams, nn.ModuleList).  Naming / ordering rules follow reference models.py:15-110 so that
    state_dict keys and `.weights` traversal (`module[0]` conv, `module[1]` BN) stay compatible."""
    hyper = module_defs.pop(0)
    channels = [int(hyper["channels"])]
    img_w, img_h = int(hyper["width"]), int(hyper["height"])
    n_cls = int(hyper["classes"])
    slope = float(hyper["leaky_slope"])
    activation = hyper["conv_activation"]
    masks = [[int(v) for v in grp.split(",")] for grp in hyper["yolo_masks"].split("|")]
    anchors_all = _read_anchor_row(hyper["train_uri"])          # opened unconditionally, like the reference (Q11)
    if vanilla_anchor:
        anchors_all = vanilla_anchor_list
    ignore = float(hyper["build_targets_ignore_thresh"])

    mods = nn.ModuleList()
    head = 0
    for i, d in enumerate(module_defs):
        seq = nn.Sequential()
        kind = d["type"]
        if kind == "convolutional":
            is_head = d["filters"] == "preyolo"                   # bias, no BN, linear (models.py:51-54)
            filters = (n_cls + 5) * len(masks[head]) if is_head else int(d["filters"])
            k = int(d["size"])
            seq.add_module("conv_%d" % i, nn.Conv2d(channels[-1], filters, k, int(d["stride"]), (k - 1) // 2, bias=is_head))
            if not is_head:
                seq.add_module("batch_norm_%d" % i, nn.BatchNorm2d(filters))
                if activation == "leaky":
                    seq.add_module("leaky_%d" % i, nn.LeakyReLU(slope))
                if activation == "ReLU":
                    seq.add_module("ReLU_%d" % i, nn.ReLU())
        elif kind == "maxpool":
            k, s = int(d["size"]), int(d["stride"])
            if k == 2 and s == 1:
                seq.add_module("_debug_padding_%d" % i, nn.ZeroPad2d((0, 1, 0, 1)))
            seq.add_module("maxpool_%d" % i, nn.MaxPool2d(k, s, (k - 1) // 2))
            filters = channels[-1]
        elif kind == "upsample":
            seq.add_module("upsample_%d" % i, nn.Upsample(scale_factor=int(d["stride"]), mode="nearest"))
            filters = channels[-1]
        elif kind == "route":
            filters = 0
            for v in (int(t) for t in d["layers"].split(",")):
                filters += channels[v + 1 if v > 0 else v]          # `channels` has the input in front (models.py:93-96)
            seq.add_module("route_%d" % i, EmptyLayer())
        elif kind == "shortcut":
            filters = channels[int(d["from"])]
            seq.add_module("shortcut_%d" % i, EmptyLayer())
        elif kind == "yolo":
            seq.add_module("yolo_%d" % i, YOLOLayer([anchors_all[v] for v in masks[head]], n_cls, img_h, img_w, ignore, activation,
                                                    xy_loss, wh_loss, object_loss, no_object_loss))
            head += 1
            filters = channels[-1]
        else:
            raise ValueError("unknown cfg section [%s]" % kind)
        mods.append(seq)
        channels.append(filters)
    return hyper, mods


class _YoloHeadFn(torch.autograd.Function):
    """Stand-alone YOLOLayer on an NCHW sample: NHWC fp32 staging + the fused head kernels."""

    @staticmethod
    def forward(ctx, layer, sample, targets):
        L = _lib.lib()
        B, ch, Gh, Gw = sample.shape
        A, C = layer.num_anchors, layer.num_classes
        dev = sample.device
        st = torch.cuda.current_stream().cuda_stream
        cp = pad8(ch)
        lg = torch.empty(B * Gh * Gw * cp, dtype=torch.float32, device=dev)
        src = sample.detach().to(torch.float32).contiguous()
        L.check(L.nchw_to_nhwc(_lib.F32, src.data_ptr(), lg.data_ptr(), B, ch, Gh, Gw, cp, cp, st), "nchw_to_nhwc")
        tg = targets.detach().to(device=dev, dtype=torch.float32).contiguous()
        anchors = layer.scaled_anchors(Gh).to(dev)
        ws = torch.empty(int(L.yolo_head_workspace_bytes(B, A, Gh, Gw)), dtype=torch.uint8, device=dev)
        out7 = torch.zeros(7, dtype=torch.float32, device=dev)
        geo = (B, tg.shape[1], A, C, Gh, Gw, float(layer.ignore_thres), float(layer.xy_loss), float(layer.wh_loss),
               float(layer.object_loss), float(layer.no_object_loss))
        L.check(L.yolo_head_train(_lib.F32, lg.data_ptr(), cp, None, 0, cp, tg.data_ptr(), anchors.data_ptr(), *geo, ws.data_ptr(),
                                  out7.data_ptr(), None, st), "yolo_head_train")
        if _CHECK_TARGETS and int(_head_err_view(ws, B, A, Gh, Gw).item()):
            raise IndexError(_BAD_TARGET_MSG)
        ctx.saved = (lg, tg, anchors, ws, geo, cp, ch)
        return out7

    @staticmethod
    def backward(ctx, gout):
        L = _lib.lib()
        lg, tg, anchors, ws, geo, cp, ch = ctx.saved
        B, Gh, Gw = geo[0], geo[4], geo[5]
        st = torch.cuda.current_stream().cuda_stream
        g = gout.contiguous()
        dl = torch.empty_like(lg)
        L.check(L.yolo_head_grad(_lib.F32, lg.data_ptr(), cp, dl.data_ptr(), cp, cp, tg.data_ptr(), anchors.data_ptr(), *geo, ws.data_ptr(),
                                 g.data_ptr(), st), "yolo_head_grad")
        ds = torch.empty(B, ch, Gh, Gw, dtype=torch.float32, device=lg.device)
        L.check(L.nhwc_to_nchw(_lib.F32, dl.data_ptr(), cp, ds.data_ptr(), B, ch, Gh, Gw, st), "nhwc_to_nchw")
        return None, ds, None


class YOLOLayer(nn.Module):
    """Detection head.  ctor argument order as in the reference (note object_loss before no_object_loss, models.py:121).
    forward(sample, targets) -> (loss, tensor(6 parts: x,y,w,h,obj,noobj)) ; forward(sample) -> [B, A*G*G, 5+C]."""

    def __init__(self, anchors, num_classes, img_height, img_width, build_targets_ignore_thresh, conv_activation, xy_loss, wh_loss,
                 object_loss, no_object_loss):
        super().__init__()
        self.anchors = anchors
        self.num_anchors = len(anchors)
        self.num_classes = num_classes
        self.bbox_attrs = 5 + num_classes
        self.image_height, self.image_width = img_height, img_width
        self.ignore_thres = build_targets_ignore_thresh
        self.xy_loss, self.wh_loss = xy_loss, wh_loss
        self.no_object_loss, self.object_loss = no_object_loss, object_loss
        self.conv_activation = conv_activation

    def stride_for(self, grid_h):
        return self.image_height / grid_h                          # cfg height, used for both axes (models.py:145)

    def scaled_anchors(self, grid_h):
        s = self.stride_for(grid_h)
        return torch.tensor([(aw / s, ah / s) for aw, ah in self.anchors], dtype=torch.float32)

    def forward(self, sample, targets=None):
        _lib.require_gpu(sample)
        if targets is not None:
            out7 = _YoloHeadFn.apply(self, sample, targets)
            return out7[0], out7[1:].detach()
        L = _lib.lib()
        B, ch, Gh, Gw = sample.shape
        st = torch.cuda.current_stream().cuda_stream
        cp = pad8(ch)
        lg = torch.empty(B * Gh * Gw * cp, dtype=torch.float32, device=sample.device)
        src = sample.detach().to(torch.float32).contiguous()
        L.check(L.nchw_to_nhwc(_lib.F32, src.data_ptr(), lg.data_ptr(), B, ch, Gh, Gw, cp, cp, st), "nchw_to_nhwc")
        rows = self.num_anchors * Gh * Gw
        out = torch.empty(B, rows, self.bbox_attrs, dtype=torch.float32, device=sample.device)
        an = self.scaled_anchors(Gh).to(sample.device)
        L.check(L.yolo_head_decode(_lib.F32, lg.data_ptr(), cp, an.data_ptr(), float(self.stride_for(Gh)), B, self.num_anchors,
                                   self.num_classes, Gh, Gw, out.data_ptr(), rows, 0, st), "yolo_head_decode")
        return out


class _DarknetTrainFn(torch.autograd.Function):
    """One autograd node for the whole network: forward = plan.fwd, backward = plan.bwd."""

    @staticmethod
    def forward(ctx, model, plan, x, targets, *params):
        plan.run_forward(x, targets)
        ctx.model, ctx.plan = model, plan
        return plan.out7.clone()

    @staticmethod
    def backward(ctx, gout):
        model, plan = ctx.model, ctx.plan
        model._run_backward(plan, gout)
        return (None, None, None, None) + (None,) * len(model._plist)


_CHECK_TARGETS = True       # (module attribute: tests may switch the one-step-late label check off)
_BAD_TARGET_MSG = ("index out of range in build_targets: a target has cx >= 1.0 or cy >= 1.0 (grid cell == grid size), where the reference "
                   "raises IndexError at utils/utils.py:262")


def _head_err_view(ws, B, A, Gh, Gw):
    """the int32 `err` word of a YOLO head workspace (csrc/yolo_head.hip: owner[B*A*Gh*Gw] | ignore[Gh*Gw] | err)"""
    return ws.view(torch.int32)[B * A * Gh * Gw + Gh * Gw:B * A * Gh * Gw + Gh * Gw + 1]


class _YoloPlan(netplan._NetPlan):
    """The Darknet plan: netplan._NetPlan + the one-step-late check of the labels the fused training heads dropped."""

    err_views = ()        # int32 one-element views of the YOLO heads' `err` words (training plans)

    def watch_head(self, ws, B, A, Gh, Gw):
        self.err_views = tuple(self.err_views) + (_head_err_view(ws, B, A, Gh, Gw),)

    def check_targets(self, block=True):
        """Raises IndexError if the targets of the LAST forward through this plan held a centre coordinate >= 1.0 (the reference's
        build_targets indexes its [B,A,G,G] tensors with gi == G there and raises, utils/utils.py:262; the fused head drops the
        target and sets a flag).  The flags ride to a pinned host word with a non-blocking copy behind every forward and are
        looked at (i) at the end of that step's backward(), behind its queued launches -- waiting for the copy (one host wait per step
        that the GPU does not see: a bad label then raises BEFORE optimizer.step(), like the reference) unless the model sets
        `strict_targets = False`, in which case the look is a query and a copy that has not landed stays pending --, (ii) at the
        start of the NEXT forward and (iii) when the plan is dropped."""
        ev = getattr(self, "_err_event", None)
        if ev is None or not _CHECK_TARGETS:
            return
        if not block and not ev.query():
            return                                           # not landed yet: the next forward (or the plan's eviction) looks again
        self._err_event = None
        ev.synchronize()
        if bool(self._err_host.any()):
            raise IndexError(_BAD_TARGET_MSG)

    def before_forward(self, targets):
        if targets is not None:
            self.check_targets()

    def after_forward(self, targets):
        if targets is not None and self.err_views and _CHECK_TARGETS:
            if getattr(self, "_err_host", None) is None:
                self._err_host = torch.zeros(len(self.err_views), dtype=torch.int32).pin_memory()
            self._err_host.copy_(torch.cat(self.err_views), non_blocking=True)
            self._err_event = torch.cuda.Event()
            self._err_event.record()



class Darknet(netplan.FlatParamsMixin, nn.Module):
    """YOLOv3 object detection model (reference: CVC-YOLOv3/models.py:222-422)."""

    def __init__(self, config_path, xy_loss, wh_loss, no_object_loss, object_loss, vanilla_anchor, precision=None):
        super().__init__()
        self.module_defs = parse_model_config(config_path)
        self.hyperparams, self.module_list = create_modules(self.module_defs, xy_loss, wh_loss, no_object_loss, object_loss, vanilla_anchor)
        h = self.hyperparams
        self.img_width, self.img_height = int(h["width"]), int(h["height"])
        self.onnx_height = int(h["onnx_height"])
        self.onnx_name = config_path.split("/")[-1].split(".")[0] + "_" + str(self.img_width) + str(self.onnx_height) + ".onnx"
        self.num_classes = int(h["classes"])
        ch = int(h["channels"])
        if ch not in (1, 3):
            print("Channels in cfg file is not set properly, making it colour")
        self.bw = ch == 1
        self.validate_uri, self.train_uri = h["validate_uri"], h["train_uri"]
        self.num_train_images, self.num_validate_images = int(h["num_train_images"]), int(h["num_validate_images"])
        self.conf_thresh, self.nms_thresh, self.iou_thresh = float(h["conf_thresh"]), float(h["nms_thresh"]), float(h["iou_thresh"])
        self.start_weights_dim = [int(v) for v in h["start_weights_dim"].split(",")]
        self.conv_activation = h["conv_activation"]
        self.xy_loss, self.wh_loss, self.no_object_loss, self.object_loss = xy_loss, wh_loss, no_object_loss, object_loss
        self.anchors = vanilla_anchor_list if vanilla_anchor else _read_anchor_row(h["train_uri"])
        self.seen = 0
        self.header_info = np.array([0, 0, 0, self.seen, 0], dtype=np.int32)
        self._stamp = (datetime.now().strftime("%B").lower(), str(datetime.now().year))
        self.precision = parse_precision(precision if precision is not None else os.environ.get("MDCV_PRECISION", "bf16"))
        self.use_graph = os.environ.get("MDCV_GRAPH", "0") == "1"
        self._plans = {}
        self.register_state_dict_pre_hook(netplan._sync_before_state_dict)   # a pipelined optimizer step may be in flight

    def __getstate__(self):
        return self._state_without_plans()

    def load_state_dict(self, *args, **kw):
        self._param_sync()
        out = super().load_state_dict(*args, **kw)
        self._params_changed()
        return out

    # ---- getters consumed by train.py / validate.py / detect.py (reference models.py:279-310)
    def get_start_weight_dim(self): return self.start_weights_dim
    def get_onnx_name(self): return self.onnx_name
    def get_bw(self): return self.bw
    def get_loss_constant(self): return [self.xy_loss, self.wh_loss, self.no_object_loss, self.object_loss]
    def get_conv_activation(self): return self.conv_activation
    def get_num_classes(self): return self.num_classes
    def get_anchors(self): return self.anchors
    def get_threshs(self): return self.conf_thresh, self.nms_thresh, self.iou_thresh
    def img_size(self): return self.img_width, self.img_height
    def get_links(self): return self.validate_uri, self.train_uri
    def num_images(self): return self.num_validate_images, self.num_train_images

    # ------------------------------------------------------------------------------------------ forward
    def forward(self, x, targets=None):
        _lib.require_gpu(x)
        if not self._flat_ok():
            self._flatten()
        if targets is not None and self.training and torch.is_grad_enabled():
            (x, targets), dp_weight = self._auto_dp_shard(x, targets)     # torchrun on the unchanged train.py: rank r's shard (parallel.enable_auto_data_parallel)
        else:
            dp_weight = None
        B, _, H, W = x.shape
        T = targets.shape[1] if targets is not None else 0
        key = (B, H, W, T, targets is not None, self.training, self.precision, x.device.index)
        plan = self._plan_lookup(key)
        if plan is None:
            plan = self._build_plan(x.device, B, H, W, T, targets is not None, self.training)
            self._plan_store(key, plan)
        if getattr(self, "_pipe_plan", None) is not None and plan is not self._pipe_plan:
            self._param_sync()               # deferred group updates of a pipelined optimizer step are only released from ITS plan's forward list
        if targets is None:
            plan.run_forward(x)
            return plan.eval_out.clone()
        if torch.is_grad_enabled() and plan.has_bwd:
            out7 = _DarknetTrainFn.apply(self, plan, x, targets, *self._plist)
        else:
            plan.run_forward(x, targets)
            out7 = plan.out7.clone()
        if dp_weight == 0.0:
            out7 = out7 * 0.0                # this rank's DataParallel chunk was empty: it joins the exchange with exact-zero gradients
        d = out7.detach()
        return (out7[0], d[1], d[2], d[3], d[4], d[5], d[6])

    # ------------------------------------------------------------------------------------------ plan
    def _build_plan(self, device, B, H, W, T, with_targets, bn_train):
        """cfg -> launch plan: graph analysis, one forward lowering per section (yolo/lower.py), then the records' backwards in reverse."""
        cin = int(self.hyperparams["channels"])
        plan, xin = _YoloPlan.begin(self, device, bn_train, B, cin, H, W, self.use_graph)
        plan.targets = torch.zeros(B, max(T, 1), 5, dtype=torch.float32, device=device)
        plan.out7 = torch.zeros(7, dtype=torch.float32, device=device)
        plan.gscale = torch.ones(1, dtype=torch.float32, device=device)
        plan.has_bwd = with_targets
        layout = lower.analyse(self.module_defs, self.module_list, cin, H, W)
        cx = lower.Lowering(plan, self, layout, xin, B, T, with_targets)          # (allocates the concat buffers)
        plan.call(plan.fwd, netplan._zero_tensor, plan.out7)
        if bn_train and plan.stats_xacc:                          # exact accumulators of the forward statistics (engine.fold_forward_xstats): one memset per forward
            plan._xacc_arena = torch.zeros(plan.stats_xacc_words, dtype=torch.int64, device=device)
            plan.keep.append(plan._xacc_arena)
            plan.call(plan.fwd, netplan._zero_tensor, plan._xacc_arena)
        if not with_targets:
            plan.eval_out = torch.zeros(B, cx.rows_total, 5 + self.num_classes, dtype=torch.float32, device=device)
        recs = []
        for i, d in enumerate(self.module_defs):
            rec = lower.FORWARD[d["type"]](cx, i, d)
            if rec is not None:
                recs.append(rec)
        if bn_train and cx.nbt:
            plan.call(plan.fwd, netplan._bump_counters, cx.nbt)
        if plan.stats_xacc:
            plan.fold_forward_xstats()     # conv -> finalize -> apply triples that survived the peepholes become two launches (csrc/exact_acc.h)
        plan.finish_pack(0)
        if with_targets:                   # backward list: mirror of the records, consumers before producers
            for r in reversed(recs):
                plan.mark_ready()
                r.backward(plan)
            plan.mark_ready()
        plan.outs = cx.outs
        plan.recs = recs
        return plan

    # ------------------------------------------------------------------------------------------ darknet .weights I/O
    def load_weights(self, weights_path, start_weight_dim):
        """Binary layout (reference models.py:339-397): int32[5] header, then for every conv in cfg order
        BN bias, BN weight, running_mean, running_var, conv weight (OIHW)  |  head: bias, weight — read from a tensor that is
        `start_weight_dim[head]` filters wide, of which the first num_filters are kept."""
        with open(weights_path, "rb") as fp:
            header = np.fromfile(fp, dtype=np.int32, count=5)
            blob = np.fromfile(fp, dtype=np.float32)
        self.header_info = header
        self.seen = header[3]
        pos, head = 0, 0
        self._param_sync()
        self._params_changed()

        def take(dst, count=None):
            nonlocal pos
            cnt = dst.numel() if count is None else count
            dst.data.copy_(torch.from_numpy(blob[pos:pos + cnt].copy()).view_as(dst))
            pos += cnt
        with torch.no_grad():
            for d, m in zip(self.module_defs, self.module_list):
                if d["type"] != "convolutional":
                    continue
                conv = m[0]
                if d["filters"] != "preyolo":
                    bn = m[1]
                    take(bn.bias); take(bn.weight); take(bn.running_mean); take(bn.running_var)
                    take(conv.weight)
                else:
                    wide = start_weight_dim[head]
                    head += 1
                    nb = conv.bias.numel()
                    conv.bias.data.copy_(torch.from_numpy(blob[pos:pos + nb].copy()))
                    pos += wide
                    per = conv.weight.numel() // nb
                    full = torch.from_numpy(blob[pos:pos + per * wide].copy()).view(wide, *conv.weight.shape[1:])
                    conv.weight.data.copy_(full[:nb])
                    pos += per * wide

    def save_weights(self, path, cutoff=-1):
        """Byte-compatible darknet .weights (reference models.py:400-422).  Under torchrun (parallel.enable_auto_data_parallel) every rank reaches
        this call of the unchanged script with identical parameters: rank 0 alone writes -- to a temporary name, renamed when complete --, and all
        ranks leave together, so a rank that loads the file right afterwards reads whole bytes (until round 5 N ranks truncated and rewrote the
        same path concurrently)."""
        from ..parallel import auto_is_writer, auto_barrier
        self._param_sync()
        if not auto_is_writer():
            auto_barrier()
            return
        tmp_path = f"{path}.tmp.{os.getpid()}"
        try:
            self._write_weights(tmp_path, cutoff)
            os.replace(tmp_path, path)
        finally:
            if os.path.exists(tmp_path):
                os.remove(tmp_path)
            auto_barrier()                                   # (also when the write failed: the other ranks are waiting in theirs)

    def _write_weights(self, path, cutoff):
        with open(path, "wb") as fp:
            self.header_info[3] = self.seen
            np.asarray(self.header_info, dtype=np.int32).tofile(fp)
            for d, m in zip(self.module_defs[:cutoff], self.module_list[:cutoff]):
                if d["type"] != "convolutional":
                    continue
                conv = m[0]
                if d["filters"] != "preyolo":
                    bn = m[1]
                    for t in (bn.bias, bn.weight, bn.running_mean, bn.running_var):
                        t.data.cpu().numpy().tofile(fp)
                else:
                    conv.bias.data.cpu().numpy().tofile(fp)
                conv.weight.data.cpu().numpy().tofile(fp)
