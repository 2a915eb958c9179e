"""Fused flat-buffer optimizers (HIP) with the torch.optim interface.

`FusedAdam(model, lr=...)` / `FusedSGD(model, lr=..., momentum=...)` update every parameter of a Darknet / KeypointNet in ONE
launch over the model's flat fp32 parameter buffer (engine side: FlatParamsMixin), instead of the 222 / 54 per-tensor
updates torch.optim performs for the reference (CVC-YOLOv3/train.py:180-187,72 ; RektNet/train_eval.py:263,72).
Update rules, defaults and `param_groups[0]["lr"]` handling (LR schedulers) follow torch.optim.Adam / SGD.

`guard=GradGuard(max_norm=..., skip_nonfinite=...)` puts two launches in front of the update (csrc/grad_guard.hip): the global
gradient norm, the clip coefficient and the decision to drop a step whose gradient is not finite are formed on the device, and the update
reads them from there.  Nothing waits for the GPU; `guard.stats()` reads the counters when somebody wants them.

`ema=WeightEMA(model, decay=...)` puts up to three launches behind the update (csrc/weight_ema.hip): an exponential moving
average of the flat parameter buffer and of the BatchNorm running statistics in one shadow buffer, which follows the guard's decision on
the device.  `with ema.applied():` swaps the averaged model in for validation and checkpoints and swaps it back.
"""
import contextlib
import ctypes
import math

import torch

from . import _lib

GUARD_CHUNK = 4096          # include/mdcv_hip.h MDCV_GRAD_GUARD_CHUNK: elements per partial sum
_BLOCK_WORDS = 9            # mdcv_grad_guard_block: 72 bytes


class GradGuard:
    """Device-side global-norm clipping and non-finite-step skipping for FusedAdam / FusedSGD (pass it as `guard=`).

    max_norm        clip the global L2 norm of the (scaled) gradient to this, torch.nn.utils.clip_grad_norm_'s rule; None / 0: no clipping
    skip_nonfinite  a step whose gradient holds a NaN or an Inf changes nothing: not a parameter, not a moment, not the bias correction
    ring            how many of the latest norms `stats()` can return

    Owns the control block (mdcv_grad_guard_block), the ring of norms behind it in the same allocation (so `stats()` is ONE host read) and
    the partial-sum scratch, sized from the flat gradient buffer at first use.  One guard serves one optimizer.

    Known limit: the guard acts between the backward and the update.  A step whose FORWARD already produced non-finite activations has
    written them into the BatchNorm running statistics before the guard sees anything."""

    def __init__(self, max_norm=None, skip_nonfinite=True, ring=1024):
        if max_norm is not None and not (max_norm >= 0 and math.isfinite(max_norm)):
            raise ValueError("GradGuard: max_norm must be None or a finite number >= 0 (0 = no clipping)")
        if int(ring) < 1:
            raise ValueError("GradGuard: ring must be >= 1")
        self.max_norm = float(max_norm) if max_norm else 0.0
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ring = int(ring)
        self._buf = None            # int64 words: the block, then the ring of fp32 norms
        self._partials = None
        self._pending = None        # counters of a checkpoint loaded before the first step
        self._seen = dict(attempted=0, applied=0, skipped=0, clipped=0)      # counters at the last summary()

    def _ensure(self, device, n):
        if self._buf is None or self._buf.device != device:
            old = self._buf
            self._buf = torch.zeros(_BLOCK_WORDS + (self.ring + 1) // 2, dtype=torch.int64, device=device)
            if old is not None:
                self._buf.copy_(old)
            if self._pending is not None:
                self._write_counters(self._pending)
                self._pending = None
        need = (n + GUARD_CHUNK - 1) // GUARD_CHUNK
        if self._partials is None or self._partials.numel() < need or self._partials.device != device:
            self._partials = torch.empty(need, dtype=torch.float64, device=device)

    @property
    def block_ptr(self):
        return self._buf.data_ptr()

    @property
    def norm(self):
        """the last measured norm: a device fp32 scalar view of the control block (a StepLog source, say); valid after the first step"""
        if self._buf is None:
            raise RuntimeError("GradGuard.norm: nothing has been measured yet")
        return self._buf[1:2].view(torch.float32)[0]

    def measure(self, gflat, grad_scale=1.0, betas=(0.0, 0.0)):
        """enqueue sumsq -> finalize over `gflat` on the current stream (what a guarded step() does in front of its update)"""
        _lib.require_gpu(gflat)
        L = _lib.lib()
        n = gflat.numel()
        self._ensure(gflat.device, n)
        s = torch.cuda.current_stream().cuda_stream
        L.check(L.grad_sumsq(gflat.data_ptr(), n, self._partials.data_ptr(), s), "grad_sumsq")
        # the betas as the update kernels see them: rounded to fp32, then widened
        b1, b2 = (ctypes.c_float(b).value for b in betas)
        L.check(L.grad_guard_finalize(self._partials.data_ptr(), (n + GUARD_CHUNK - 1) // GUARD_CHUNK, float(grad_scale), self.max_norm,
                                      int(self.skip_nonfinite), b1, b2, self._buf.data_ptr(), self._buf[_BLOCK_WORDS:].data_ptr(), self.ring, s),
                "grad_guard_finalize")

    @staticmethod
    def _parse(words):
        """the block's fields from its 9 int64 words on the host"""
        f = words[:_BLOCK_WORDS].view(torch.float32)
        i = words[:_BLOCK_WORDS].view(torch.int32)
        return dict(sumsq=float(words[:1].view(torch.float64)[0]), norm=float(f[2]), coef=float(f[3]), scale=float(f[4]), bc1=float(f[5]),
                    bc2_sqrt=float(f[6]), max_norm=float(f[7]), finite=int(i[8]), apply=int(i[9]), attempted=int(words[5]),
                    applied=int(words[6]), skipped=int(words[7]), clipped=int(words[8]))

    def stats(self):
        """ONE host read (it waits for the work queued so far): the block's fields (`norm` the last one, `max_norm` the largest finite one)
        and `norms`, the ring's norms in step order -- the latest min(attempted, ring) of them; a non-finite step's norm is nan or inf"""
        if self._buf is None:
            d = dict(sumsq=0.0, norm=0.0, coef=1.0, scale=1.0, bc1=0.0, bc2_sqrt=0.0, max_norm=0.0, finite=1, apply=1, attempted=0, applied=0,
                     skipped=0, clipped=0, norms=[])
            d.update(self._pending or {})
            return d
        host = self._buf.cpu()
        d = self._parse(host)
        hist = host[_BLOCK_WORDS:].view(torch.float32)[:self.ring]
        a = d["attempted"]
        k = min(a, self.ring)
        d["norms"] = [float(hist[j % self.ring]) for j in range(a - k, a)]
        return d

    def summary(self):
        """`stats()` plus what happened since the last summary(): `steps`, `epoch_clipped`, `epoch_skipped`, and the `epoch_max` / `epoch_mean`
        of the finite norms among those steps that are still in the ring (the training loops' one line per epoch)"""
        d = self.stats()
        steps = d["attempted"] - self._seen["attempted"]
        d["steps"] = steps
        d["epoch_clipped"] = d["clipped"] - self._seen["clipped"]
        d["epoch_skipped"] = d["skipped"] - self._seen["skipped"]
        fin = [x for x in d["norms"][max(0, len(d["norms"]) - steps):] if math.isfinite(x)] if steps > 0 else []
        d["epoch_max"] = max(fin) if fin else float("nan")
        d["epoch_mean"] = sum(fin) / len(fin) if fin else float("nan")
        self._seen = {k: d[k] for k in self._seen}
        return d

    def summary_line(self, label_prefix, epoch):
        d = self.summary()
        return (f"{label_prefix} Epoch: {epoch}, grad norm max {d['epoch_max']:.4g} mean {d['epoch_mean']:.4g}, clipped {d['epoch_clipped']}, "
                f"skipped {d['epoch_skipped']} of {d['steps']} steps")

    def _write_counters(self, c):
        w = torch.tensor([int(c.get(k, 0)) for k in ("attempted", "applied", "skipped", "clipped")], dtype=torch.int64)
        self._buf[5:9].copy_(w)
        self._buf[3:4].view(torch.float32)[1:2].copy_(torch.tensor([float(c.get("max_norm", 0.0))], dtype=torch.float32))
        self._seen = {k: int(c.get(k, 0)) for k in self._seen}

    def state_dict(self):
        """the counters and the largest norm (one host read): a resumed run bias-corrects with the APPLIED count"""
        d = self.stats()
        return {k: d[k] for k in ("attempted", "applied", "skipped", "clipped", "max_norm")}

    def load_state_dict(self, sd):
        if self._buf is None:
            self._pending = dict(sd)
            self._seen = {k: int(sd.get(k, 0)) for k in self._seen}
        else:
            self._write_counters(sd)


_EMA_BLOCK_WORDS = 3        # mdcv_ema_block: 24 bytes


def ema_decay_at(decay, warmup, t):
    """the decay of update number `t` (0-based) as mdcv_ema_advance forms it: min((double)(float)decay, (1 + t) / (warmup + t)) -> float"""
    d64 = min(float(ctypes.c_float(decay).value), (1.0 + float(t)) / (float(warmup) + float(t)))
    return ctypes.c_float(d64).value


class WeightEMA:
    """An exponential moving average of a Darknet's / KeypointNet's weights and BatchNorm running statistics, kept on the device.

    decay   the decay d of `e = e + (1 - d) * (p - e)` once the warm-up is over; 0 <= decay < 1
    warmup  integer >= 1: update number t (0-based) uses d_t = min(decay, (1 + t) / (warmup + t)), so the first updates follow the
            weights closely; warmup = 1: d_t = decay from the first update

    Pass it to `FusedAdam(..., ema=)` / `FusedSGD(..., ema=)`, whose `step()` then calls `update()` behind the parameter update with
    their guard -- a step the guard dropped leaves the average and its update count alone, decided on the device.  Behind a torch optimizer
    call `update()` yourself after `optimizer.step()`.  `with ema.applied():` exchanges live and averaged values in place for validation,
    detection, `save_weights` and `state_dict`, and exchanges them back on exit.

    The shadow is ONE fp32 buffer: the model's flat parameter layout (same offsets, padding 0), then every BatchNorm `running_mean` /
    `running_var` in module order, each padded to 4 elements.  Integer buffers (`num_batches_tracked`) are neither averaged nor swapped.
    It is a copy of the live values at construction and follows a re-flatten of the model (`.to(device)`, re-pointed parameters) as long
    as the layout's size is unchanged.

    Limits: without a guard a NaN that reaches the parameters reaches the average and stays there -- train with
    `GradGuard(skip_nonfinite=True)`.  The guard acts on the optimizer step: the BatchNorm statistics of a dropped step's forward were
    written before it saw anything, and the next applied update averages them in.  Under data parallel every rank computes the same
    average from the same all-reduced update: nothing is communicated."""

    def __init__(self, model, decay=0.9999, warmup=10):
        if not hasattr(model, "flat_parameters"):
            raise TypeError("WeightEMA takes the model (Darknet / KeypointNet), not a parameter list")
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not (0.0 <= decay < 1.0) or ctypes.c_float(decay).value >= 1.0:
            raise ValueError("WeightEMA: decay must be a number with 0 <= decay < 1 (as fp32 too)")
        if isinstance(warmup, bool) or not isinstance(warmup, int) or warmup < 1:
            raise ValueError("WeightEMA: warmup must be an integer >= 1")
        self.model = model
        self.decay = float(decay)
        self.warmup = int(warmup)
        self._applied = False
        self._shadow = None         # built at first use on the device (a model still on the host has no device layout yet)
        self._blk = None            # int64 words of mdcv_ema_block
        self._table = None          # [S, 3] int64: source address, shadow offset, length
        self._srcs = None
        self._pending = None        # a state_dict loaded before the first use
        self._bn = None
        if next(model.parameters()).is_cuda:
            self._follow(model.flat_parameters()[0])

    # ---- layout
    def _stat_tensors(self, model):
        """every BatchNorm's running_mean and running_var, in module order (the module list is walked once per model; the tensors are
        looked up each time: `.to(device)` replaces them)"""
        if model is self.model:
            if self._bn is None:
                self._bn = self._bn_modules(model)
            mods = self._bn
        else:
            mods = self._bn_modules(model)
        out = []
        for m in mods:
            out.append(m._buffers["running_mean"])
            out.append(m._buffers["running_var"])
        return out

    @staticmethod
    def _bn_modules(model):
        return [m for m in model.modules()
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m._buffers.get("running_mean") is not None]

    def _build_table(self, stats, n):
        rows, off = [], n
        for t in stats:
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("WeightEMA: BatchNorm running statistics must be contiguous fp32 tensors")
            rows.append((t.data_ptr(), off, t.numel()))
            off += (t.numel() + 3) & ~3
        return rows, off

    def _follow(self, pflat):
        """brings the shadow, the block and the segment table in line with the model's current flat buffer and statistics"""
        _lib.require_gpu(pflat)
        n = pflat.numel()
        stats = self._stat_tensors(self.model)
        srcs = [t.data_ptr() for t in stats]
        if self._shadow is None:
            rows, total = self._build_table(stats, n)
            if self._pending is not None and self._pending["shadow"].numel() != total:
                raise ValueError(f"EMA state holds a shadow of {self._pending['shadow'].numel()} elements, this model's layout (flat parameters + "
                                 f"BatchNorm statistics) has {total}: the state belongs to another layout")
            self._n, self._total = n, total
            self._shadow = torch.zeros(total, dtype=torch.float32, device=pflat.device)
            self._blk = torch.zeros(_EMA_BLOCK_WORDS, dtype=torch.int64, device=pflat.device)
            self._set_table(rows, srcs, pflat.device)
            if self._pending is not None:
                self._load(self._pending)
                self._pending = None
            else:
                self._copy_live(pflat, stats)
            return
        if n != self._n:
            raise ValueError(f"EMA shadow holds {self._n} flat parameter elements ({self._total} with the BatchNorm statistics), the model's flat "
                             f"parameter buffer has {n}: the shadow belongs to another parameter layout")
        if self._shadow.device != pflat.device:
            self._shadow, self._blk = self._shadow.to(pflat.device), self._blk.to(pflat.device)
            self._srcs = None
        if srcs != self._srcs:
            rows, total = self._build_table(stats, n)
            if total != self._total:
                raise ValueError(f"EMA shadow holds {self._total} elements, the model's layout (flat parameters + BatchNorm statistics) has {total}: "
                                 "the shadow belongs to another layout")
            self._set_table(rows, srcs, pflat.device)

    def _set_table(self, rows, srcs, device):
        self._srcs = srcs
        self._table = torch.tensor(rows, dtype=torch.int64).reshape(-1, 3).to(device)
        self._rows = rows

    def _copy_live(self, pflat, stats):
        self._shadow[:self._n].copy_(pflat)
        for (_, off, ln), t in zip(self._rows, stats):
            self._shadow[off:off + ln].copy_(t.reshape(-1))

    def _layout(self):
        pflat = self.model.flat_parameters()[0]                 # (orders the current stream behind a pipelined update in flight)
        self._follow(pflat)
        return pflat

    # ---- launches
    def _check_free(self, what):
        if self._applied:
            raise RuntimeError(f"WeightEMA.{what}: the averaged weights are swapped into the model (inside `applied()`); leave it first")

    def _advance(self, L, guard, s):
        gp = None if guard is None or guard._buf is None else guard.block_ptr
        L.check(L.ema_advance(self._blk.data_ptr(), gp, self.decay, self.warmup, s), "ema_advance")

    def _update_segments(self, L, s):
        L.check(L.ema_update_segments(self._shadow.data_ptr(), self._total, self._table.data_ptr(), len(self._rows), self._blk.data_ptr(), s),
                "ema_update_segments")

    def _enqueue(self, L, pflat, guard, s):
        """advance -> flat update -> segment update on stream `s` (what update() does; the optimizers call it with the buffer they hold)"""
        self._advance(L, guard, s)
        L.check(L.ema_update(self._shadow.data_ptr(), pflat.data_ptr(), self._n, self._blk.data_ptr(), s), "ema_update")
        self._update_segments(L, s)

    @torch.no_grad()
    def update(self, guard=None):
        """enqueue one update on the current stream: three launches, no host read.  `guard`: the GradGuard whose decision on the latest
        step this update follows (None: apply)."""
        self._check_free("update")
        pflat = self._layout()
        self._enqueue(_lib.lib(), pflat, guard, torch.cuda.current_stream().cuda_stream)

    def _swap(self):
        L = _lib.lib()
        pflat = self._layout()
        s = torch.cuda.current_stream().cuda_stream
        L.check(L.ema_swap(self._shadow.data_ptr(), pflat.data_ptr(), self._n, s), "ema_swap")
        L.check(L.ema_swap_segments(self._shadow.data_ptr(), self._total, self._table.data_ptr(), len(self._rows), s), "ema_swap_segments")
        self.model._params_changed()                            # the next forward re-packs; a pack done ahead is not trusted

    @contextlib.contextmanager
    def applied(self):
        """the averaged weights and BatchNorm statistics are the model's inside the block (two launches in, two out; not re-entrant)"""
        self._check_free("applied")
        with torch.no_grad():
            self._swap()
        self._applied = True
        try:
            yield self
        finally:
            with torch.no_grad():
                self._swap()
            self._applied = False

    @torch.no_grad()
    def copy_to(self, model=None):
        """make the averaged values permanent: the model's parameters and BatchNorm statistics become the shadow's (default: this EMA's
        model; another model must have the same layout)"""
        self._check_free("copy_to")
        self._layout()
        model = self.model if model is None else model
        pflat = model.flat_parameters()[0]
        stats = self._stat_tensors(model)
        rows, total = self._build_table(stats, pflat.numel())
        if pflat.numel() != self._n or total != self._total:
            raise ValueError(f"EMA shadow holds {self._total} elements ({self._n} flat), the target model's layout has {total} ({pflat.numel()} flat)")
        pflat.copy_(self._shadow[:self._n])
        for (_, off, ln), t in zip(rows, stats):
            t.reshape(-1).copy_(self._shadow[off:off + ln])
        model._params_changed()

    @torch.no_grad()
    def reset(self):
        """the shadow becomes a copy of the live values again and the update count 0"""
        self._check_free("reset")
        pflat = self._layout()
        self._copy_live(pflat, self._stat_tensors(self.model))
        self._blk.zero_()

    # ---- reading
    @property
    def updates(self):
        """updates applied so far (ONE host read; it waits for the work queued so far)"""
        if self._blk is None:
            return int(self._pending["updates"]) if self._pending is not None else 0
        return int(self._blk[0])

    @property
    def shadow(self):
        """the shadow buffer (flat parameter layout, then the BatchNorm segments)"""
        self._layout()
        return self._shadow

    def block(self):
        """the control block's fields (one host read)"""
        if self._blk is None:
            return dict(updates=self.updates, d=0.0, omd=0.0, apply=0)
        w = self._blk.cpu()
        f, i = w.view(torch.float32), w.view(torch.int32)
        return dict(updates=int(w[0]), d=float(f[2]), omd=float(f[3]), apply=int(i[4]))

    def averaged_state_dict(self):
        """{name: tensor} of the averaged parameters and BatchNorm statistics under the model's `state_dict()` names (views of the shadow;
        not inside `applied()`, where the shadow holds the live values)"""
        self._check_free("averaged_state_dict")
        self._layout()
        out = {}
        for name, p in self.model.named_parameters():
            off, n = self.model._goff[id(p)]
            out[name] = self._shadow[off:off + n].view(p.shape)
        ptr2row = {r[0]: r for r in self._rows}
        for name, b in self.model.named_buffers():
            r = ptr2row.get(b.data_ptr())
            if r is not None and b.dtype == torch.float32 and b.numel() == r[2]:
                out[name] = self._shadow[r[1]:r[1] + r[2]].view(b.shape)
        return out

    def summary_line(self, label_prefix, epoch):
        """the training loops' one line per checkpoint (one host read: the update count; the decay follows from it)"""
        u = self.updates
        d = ema_decay_at(self.decay, self.warmup, u - 1) if u > 0 else 0.0
        return f"{label_prefix} Epoch: {epoch}, weight EMA: {u} updates, decay {d:.6g} (target {self.decay:.6g}, warmup {self.warmup})"

    def state_dict(self):
        """the shadow, the update count (one host read), decay and warmup"""
        self._check_free("state_dict")
        if self._shadow is None:
            if self._pending is not None:
                return dict(self._pending)
            raise RuntimeError("WeightEMA.state_dict: the model is not on the device yet, there is no average")
        self._layout()
        return {"shadow": self._shadow.clone(), "updates": self.updates, "decay": self.decay, "warmup": self.warmup}

    def _load(self, sd):
        self._shadow.copy_(sd["shadow"])
        self._blk.zero_()
        self._blk[0:1].copy_(torch.tensor([int(sd["updates"])], dtype=torch.int64))

    def load_state_dict(self, sd):
        self._check_free("load_state_dict")
        decay, warmup = float(sd.get("decay", self.decay)), int(sd.get("warmup", self.warmup))
        if not (0.0 <= decay < 1.0) or warmup < 1:
            raise ValueError("WeightEMA.load_state_dict: decay must lie in [0, 1) and warmup must be >= 1")
        if self._shadow is None and not next(self.model.parameters()).is_cuda:
            self._pending = dict(sd)                            # (its size is checked when the layout exists)
        else:
            self._layout()
            if sd["shadow"].numel() != self._total:
                raise ValueError(f"EMA state holds a shadow of {sd['shadow'].numel()} elements, this model's layout (flat parameters + BatchNorm "
                                 f"statistics) has {self._total}: the state belongs to another layout")
            self._load(sd)
        self.decay, self.warmup = decay, warmup


def grad_norm(model, grad_scale=1.0):
    """The global L2 norm of the model's gradient times |grad_scale|: a device fp32 scalar, through the guard's two launches (the sum of
    squares in fp64, in a fixed order) on the current stream.  No host wait."""
    _lib.require_gpu()
    _, gflat = model.flat_parameters()
    _fold_grads(model)
    g = GradGuard(ring=1)
    g.measure(gflat, grad_scale)
    return g.norm


def _fold_grads(model):
    """gradients normally ARE views of the flat gradient buffer (written in place by the backward plan); fold in anything that is not"""
    for p in model._plist:
        v = model._grad_view(p)
        if p.grad is None:
            v.zero_()
        elif p.grad.data_ptr() != v.data_ptr():
            v.copy_(p.grad)


class _FlatOptimizer(torch.optim.Optimizer):
    def __init__(self, model, defaults):
        if not hasattr(model, "flat_parameters"):
            raise TypeError("Fused optimizers take the model (Darknet / KeypointNet), not a parameter list")
        self.model = model
        super().__init__(list(model.parameters()), defaults)
        self._step = 0
        self._state_bufs = None
        self.guard = None
        self.ema = None

    def _take_ema(self, ema):
        if ema is not None and not isinstance(ema, WeightEMA):
            raise TypeError("ema= takes a mdcv.optim.WeightEMA")
        if ema is not None and ema.model is not self.model:
            raise ValueError("ema= was built for another model")
        self.ema = ema

    def _flat(self, nstate):
        if self.ema is not None:
            self.ema._check_free("update")                   # a step while the averaged weights are swapped in would train THEM
        pflat, gflat = self.model.flat_parameters()
        if self._state_bufs is None:
            self._state_bufs = [torch.zeros_like(pflat) for _ in range(nstate)]
        elif self._state_bufs[0].numel() != pflat.numel() or len(self._state_bufs) != nstate:
            # moments of another flat layout (a checkpoint written before parameters were padded to 16-byte boundaries, another model): zeroing them
            # while keeping `step` would resume with wrong bias correction and no sign of it
            raise ValueError(f"optimizer state holds {len(self._state_bufs)} buffer(s) of {self._state_bufs[0].numel()} elements, the model's flat "
                             f"parameter buffer has {pflat.numel()} ({nstate} expected): the state belongs to another parameter layout")
        elif self._state_bufs[0].device != pflat.device:
            self._state_bufs = [b.to(pflat.device) for b in self._state_bufs]
        _fold_grads(self.model)
        return pflat, gflat

    def state_dict(self):
        sd = {"step": self._step, "state": [b.clone() for b in (self._state_bufs or [])], "param_groups": [
            {k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}
        if self.guard is not None:
            sd["guard"] = self.guard.state_dict()            # (one host read, at checkpoint time)
        if self.ema is not None:
            sd["ema"] = self.ema.state_dict()                # (one more)
        return sd

    def load_state_dict(self, sd):
        if sd["state"]:
            n = self.model.flat_parameters()[0].numel()
            bad = [int(b.numel()) for b in sd["state"] if b.numel() != n]
            if bad:
                raise ValueError(f"optimizer checkpoint holds flat state of {bad[0]} elements, this model's flat parameter buffer has {n}: it was "
                                 "written for another parameter layout (e.g. before parameters were padded to 16-byte boundaries)")
            self._state_bufs = [b.clone() for b in sd["state"]]
        self._step = sd["step"]
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update(s)
        if self.guard is not None:
            # a checkpoint written without a guard: every one of its steps was applied
            self.guard.load_state_dict(sd.get("guard") or dict(attempted=sd["step"], applied=sd["step"]))
        if self.ema is not None and sd.get("ema") is not None:
            self.ema.load_state_dict(sd["ema"])


class FusedAdam(_FlatOptimizer):
    """`pipeline=True`: the update is cut into a few forward-ordered groups of whole layers, each followed by the re-pack of
    that group's conv operands, all on a parameter stream; `step()` returns at once and the NEXT forward of the training plan
    waits group by group (engine.Plan.ensure_param_groups).  The ~0.7 ms of HBM-bound optimizer + pack work of a YOLOv3 step then
    runs under the MFMA-bound first layers of the following forward instead of in front of it.  Same arithmetic, same order of
    operations per element; only the stream differs.  Readers of the parameters go through `model.flat_parameters()` /
    `synchronize()`, which order the current stream behind the update."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, pipeline=False, guard=None, ema=None):
        super().__init__(model, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.pipeline = pipeline
        self.guard = guard
        self._take_ema(ema)
        self._pstream = None

    def synchronize(self):
        """current stream waits for a pipelined update still in flight"""
        self.model._param_sync()

    def zero_grad(self, set_to_none=True):
        if not set_to_none:
            self.model._param_sync()       # the in-flight update still reads the gradient buffer
        super().zero_grad(set_to_none=set_to_none)

    def _pipelined(self, L, plan, groups, pflat, gflat, m, v, g, grad_scale):
        model = self.model
        cur = torch.cuda.current_stream()
        if self._pstream is None:
            from .engine import checked_stream
            self._pstream = checked_stream(pflat.device, [cur], "param")      # (checked to run beside the current stream)
        ps = self._pstream
        # Weight EMA: the advance (which reads the guard's decision and writes the EMA block) and the BatchNorm segments go on `cur`, in front
        # of the wait_stream; each group's range update goes behind that group's update and re-pack on the parameter stream, in front of its
        # event -- it overlaps the next forward as the update does, and `_param_sync()` covers it with the same events.  The EMA block is
        # still this step's when the late groups run, by the argument written for the guard block below: the next advance is enqueued by
        # the next step() (or update()), whose `flat_parameters()` -> `_param_sync()` first launches every pending group and waits for it.
        ema = self.ema
        if ema is not None:
            ema._follow(pflat)
            ema._advance(L, self.guard, cur.cuda_stream)
            ema._update_segments(L, cur.cuda_stream)
            ep, eblk = ema._shadow.data_ptr(), ema._blk.data_ptr()
        ps.wait_stream(cur)                                  # gradients final (backward, side stream, all-reduce all joined `cur`)
        for pl in model._plans.values():
            pl.owner = model
        pp, gp, mp, vp = pflat.data_ptr(), gflat.data_ptr(), m.data_ptr(), v.data_ptr()
        tab = plan.pack_table.data_ptr()
        hyp = (self._step, float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), float(grad_scale))
        # Guarded: every group reads ONE control block, written by the finalize that step() put on `cur` in front of the wait_stream above.
        # The late groups run from the next forward, and the block must still be this step's when they do.  It is: the next finalize is
        # enqueued by the next step(), whose `_flat()` -> `flat_parameters()` -> `_param_sync()` first launches every group still pending
        # and makes `cur` wait for every group's event -- and in the training loop already the next forward has waited for every group
        # in front of the backward that the next step() follows.  So no double buffering.  A skipped group's pack_weights_batched re-packs
        # unchanged weights into the operands the forward reads: the same bytes as before, a little wasted bandwidth on a rare step.
        blk = None if self.guard is None else self.guard.block_ptr
        ghyp = hyp[1:6]

        def make(k, lo, hi, first, nl):
            def launch(after_stream):
                if after_stream is not None:                 # start only when `after_stream` has reached this point on the GPU
                    gate = torch.cuda.Event()
                    gate.record(after_stream)
                    ps.wait_event(gate)
                with torch.cuda.stream(ps):
                    s = ps.cuda_stream
                    if blk is None:
                        L.check(L.adam_step(pp + 4 * lo, gp + 4 * lo, mp + 4 * lo, vp + 4 * lo, hi - lo, *hyp, s), "adam_step")
                    else:
                        L.check(L.adam_step_guarded(pp + 4 * lo, gp + 4 * lo, mp + 4 * lo, vp + 4 * lo, hi - lo, blk, *ghyp, s), "adam_step_guarded")
                    L.check(L.pack_weights_batched(plan.dtype, tab + 72 * first, nl, plan.pack_eq_taps, s), "pack_weights_batched")
                    if ema is not None:                      # behind the pack: the EMA is the group's last reader of p (non-temporal loads)
                        L.check(L.ema_update(ep + 4 * lo, pp + 4 * lo, hi - lo, eblk, s), "ema_update")
                    ev = torch.cuda.Event()
                    ev.record(ps)
                    plan._group_events[k] = ev
            return launch
        for k, (lo, hi, first, nl) in enumerate(groups):
            fn = make(k, lo, hi, first, nl)
            if k < 2:
                fn(None)                                     # the first layers' (small) groups at once
            else:
                plan._pending_updates[k] = fn                # the rest from the forward list, two groups ahead of their use
        plan._packed_ahead = True
        model._params_changed()                                     # every other plan's packed operands are stale from here on
        plan._packed_version = model._param_epoch                   # (load_weights / load_state_dict bump the epoch too: this pack is then redone)
        plan._packed_tversion = model._param_versions()             # (in-place edits of a parameter by user code bump ITS version counter)
        model._pipe_plan = plan

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        _lib.require_gpu()
        L = _lib.lib()
        g = self.param_groups[0]
        pflat, gflat = self._flat(2)
        m, v = self._state_bufs
        self._step += 1
        if self.guard is not None:
            self.guard.measure(gflat, grad_scale, g["betas"])                # sumsq -> finalize on the current stream; the update reads the block
        plan = getattr(self.model, "_last_train_plan", None)
        if self.pipeline and plan is not None and not plan.use_graph and pflat.is_cuda and getattr(plan, "pack_table", None) is not None:
            groups = plan.ensure_param_groups(pflat)
            if groups:
                self._pipelined(L, plan, groups, pflat, gflat, m, v, g, grad_scale)
                return
        s = torch.cuda.current_stream().cuda_stream
        if self.guard is not None:
            L.check(L.adam_step_guarded(pflat.data_ptr(), gflat.data_ptr(), m.data_ptr(), v.data_ptr(), pflat.numel(), self.guard.block_ptr,
                                        float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                                        s), "adam_step_guarded")
        else:
            L.check(L.adam_step(pflat.data_ptr(), gflat.data_ptr(), m.data_ptr(), v.data_ptr(), pflat.numel(), self._step, float(g["lr"]),
                                float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), float(grad_scale),
                                s), "adam_step")
        if self.ema is not None:
            self.ema._follow(pflat)
            self.ema._enqueue(L, pflat, self.guard, s)


class FusedSGD(_FlatOptimizer):
    def __init__(self, model, lr=1e-3, momentum=0.0, weight_decay=0.0, guard=None, ema=None):
        super().__init__(model, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))
        self.guard = guard
        self._take_ema(ema)

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        _lib.require_gpu()
        L = _lib.lib()
        g = self.param_groups[0]
        pflat, gflat = self._flat(1)
        self._step += 1
        s = torch.cuda.current_stream().cuda_stream
        if self.guard is not None:
            self.guard.measure(gflat, grad_scale)
            L.check(L.sgd_step_guarded(pflat.data_ptr(), gflat.data_ptr(), self._state_bufs[0].data_ptr(), pflat.numel(), self.guard.block_ptr,
                                       float(g["lr"]), float(g["momentum"]), float(g["weight_decay"]), s), "sgd_step_guarded")
        else:
            L.check(L.sgd_step(pflat.data_ptr(), gflat.data_ptr(), self._state_bufs[0].data_ptr(), pflat.numel(), self._step, float(g["lr"]),
                               float(g["momentum"]), float(g["weight_decay"]), float(grad_scale), s), "sgd_step")
        if self.ema is not None:
            self.ema._follow(pflat)
            self.ema._enqueue(L, pflat, self.guard, s)
