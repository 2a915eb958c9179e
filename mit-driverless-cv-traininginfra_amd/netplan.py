"""Network-agnostic plan running and flat parameters: what Darknet, KeypointNet and the stand-alone ResNet block share.

`_NetPlan` is engine.Plan plus the per-network I/O buffers and the run_* entry points (side-stream scheduling of weight gradients,
fork-on-dispatch, deferred slab reduces, hipGraph replay); `FlatParamsMixin` keeps a model's parameters and gradients in two flat
buffers and owns its plan cache.  Nothing here knows a network: a model lowers itself into a `_NetPlan` (sub)class it starts with
`begin()`.
"""
import ctypes
import os

import torch

from . import _lib
from .engine import Plan, side_stream


_EVAL_FUSE = True           # inference: conv + BatchNorm(running stats) + activation in one launch (module attribute; False: two-pass plans)


class _NetPlan(Plan):
    """engine.Plan + the per-network I/O buffers and the run_* entry points."""

    @classmethod
    def begin(cls, owner, device, bn_train, B, C, H, W, use_graph):
        """A plan for `owner` (a FlatParamsMixin model) whose NCHW fp32 input [B, C, H, W] is converted by the one `pre` entry.
        -> (plan, input TNode)"""
        plan = cls(device, owner.precision, bn_train, grad_sink=owner._grad_view)
        plan.owner = owner
        plan.grad_offset = lambda p: owner._goff[id(p)][0]
        plan.use_graph = use_graph
        plan.pre = []
        xin, plan.in_holder = plan.emit_input(B, C, H, W)
        plan.pre.append(plan.fwd.pop())                      # the NCHW->NHWC edge stays outside any captured graph
        plan.targets = None
        return plan, xin

    # hooks of networks that check their inputs on the device (Darknet's labels, yolo/models.py); nothing to do here
    def check_targets(self, block=True): pass
    def before_forward(self, targets): pass
    def after_forward(self, targets): pass

    def run_forward(self, x, targets=None):
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        self.before_forward(targets)
        self.in_holder["src"] = x
        if targets is not None:
            self.targets.copy_(targets.reshape(self.targets.shape), non_blocking=True)
        st = torch.cuda.current_stream().cuda_stream
        self.run(self.pre, st)
        if self.use_graph:
            self._graphed("fwd")
        else:
            self.run(self.fwd, st)
        self.after_forward(targets)

    def _graphed(self, which):
        """Replay (first call: warm run + capture) a launch list as a hipGraph.  Capture is illegal on the legacy default
        stream, so graph mode runs on a side stream fenced against the caller's stream on both sides."""
        cur = torch.cuda.current_stream()
        if getattr(self, "_gstream", None) is None:
            self._gstream = torch.cuda.Stream(device=self.device)
            self._graphs = {}
        gs = self._gstream
        gs.wait_stream(cur)
        with torch.cuda.stream(gs):
            key = (which, getattr(self, "flags", None))
            g = self._graphs.get(key)
            lst = self.fwd if which == "fwd" else self.bwd
            if g is None:
                self.run(lst, gs.cuda_stream)                          # warm run (function attributes, lazy buffers)
                self._graphs[key] = self.capture(which, gs.cuda_stream)
            else:
                self.L.check(self.L.graph_launch(g, gs.cuda_stream), "graph_launch")
        cur.wait_stream(gs)

    # Weight gradients are leaves of the backward dependency chain (only the optimizer / the gradient exchange read them), so
    # they run on a side stream: the MFMA-bound wgrad kernels of layer L overlap the HBM-bound BatchNorm passes and the
    # latency-bound tiny kernels of layers L-1, L-2, ... on the main stream.  Every buffer of a plan is its own allocation (no
    # pooling), so the only ordering needed is "dY(L), X(L) ready" (side waits on main) and "all gradients done" (main waits on
    # side at the end; the data-parallel reducer's comm stream waits on both).
    overlap_wgrad = os.environ.get("MDCV_WGRAD_STREAM", "1") == "1"
    fork_device_scope = 1

    def side(self):
        if getattr(self, "_side", None) is None:
            self._side = side_stream(self.device)           # one per device, checked to overlap with the current stream (engine.side_stream)
        return self._side

    def run_bwd_list(self):
        """The backward launch list on the current stream, weight gradients on the side stream (see above)."""
        cur = torch.cuda.current_stream()
        if not self.overlap_wgrad or "run" in self.__dict__:                   # (bench.py's per-kernel timing swaps `run`)
            self.run(self.bwd, cur.cuda_stream)
            return
        side = self.side()
        st, ss = cur.cuda_stream, side.cuda_stream
        L = self.L
        fork, used = L.stream_fork, False                      # (one ring event, device-scope release; torch's wait_stream builds an Event per call)
        rkey = (len(self.bwd), self.fork_on_dispatch, self.defer_slab_reduce)
        if self.__dict__.get("_bwd_roles_key") != rkey:      # (A/B scripts flip the two switches after the first backward)
            self._bwd_roles, self._bwd_roles_key = self._classify_bwd(), rkey
        roles = self._bwd_roles
        ev = ctypes.c_void_p()
        armed = False
        pending = []                                           # deferred slab reduces (role 3): they ride behind the NEXT fork
        overlapped_dp = self.on_ready is not None

        def flush():
            for pfn, pargs in pending:
                prc = pfn(*pargs, ss)
                if prc:
                    raise _lib.MdcvError(f"{getattr(pfn, '__name__', pfn)} returned {prc}")
            del pending[:]
        dp_red = getattr(self.on_ready, "__self__", None) if overlapped_dp else None
        for (fn, args), role in zip(self.bwd, roles):
            if role == 3 and (not overlapped_dp or dp_red is not None):   # slab reduce of a one-launch 1x1 backward: its producer is already in the main
                pending.append((fn, args))                     # queue, so ANY later fork orders it; no fork (and no 5 us of main queue) of its own
                continue
            if pending and dp_red is not None and getattr(fn, "__name__", "") == "grad_ready" and dp_red.would_fire(fn.low_water):
                # data parallel: this marker starts the all-reduce of a bucket, which waits for the side stream -- the deferred slab reduces of the
                # bucket's layers must be IN that stream first (about eight buckets per YOLOv3 step: eight forks instead of one per 1x1 layer)
                L.check(fork(st, ss, self.fork_device_scope), "stream_fork")
                flush()
                used = True
            if role >= 2:                                      # a weight gradient: side stream, behind "dY(L), X(L) ready"
                if armed:
                    L.check(L.stream_fork_wait(ss, ev), "stream_fork_wait")           # the kernel in front of it carried the event
                    armed = False
                else:
                    L.check(fork(st, ss, self.fork_device_scope), "stream_fork")
                if pending:
                    flush()
                rc = fn(*args, ss)
                used = True
            else:
                if role == 1:                                  # single-kernel call in front of a weight gradient: its dispatch carries the event
                    L.check(L.stream_fork_arm(st, self.fork_device_scope, ctypes.byref(ev)), "stream_fork_arm")
                    armed = True
                rc = fn(*args, st)
            if rc:
                if armed:                                      # the armed call failed before it launched: take the event back, or the next unrelated
                    L.stream_fork_wait(ss, ev)                 # launch of this thread would carry it as its stop event (fork_wait clears a pending arm)
                raise _lib.MdcvError(f"{getattr(fn, '__name__', fn)} returned {rc}")
        if pending:
            L.check(fork(st, ss, self.fork_device_scope), "stream_fork")
            flush()
            used = True
        if used:
            L.check(fork(ss, st, self.fork_device_scope), "stream_fork")              # main waits for "all gradients done"

    # An event record between two dependent kernels of the main queue costs that queue ~7 us (rocprofv3 trace, round 5: 7.2 - 7.8 us between a
    # kernel and its successor wherever a fork sat between them, 0.0 - 0.6 us elsewhere; 71 forks per YOLOv3 backward).  Where the call in
    # front of a weight gradient is ONE kernel launch, that kernel's own dispatch packet carries the event (mdcv_stream_fork_arm) instead.
    fork_on_dispatch = True
    defer_slab_reduce = True           # the slab reduces of the one-launch 1x1 backward wait for the next weight gradient's fork (32 forks fewer per YOLOv3 step)

    def _classify_bwd(self):
        """per backward-list entry: 2 = weight gradient (side stream), 3 = slab reduce that may wait for the next fork, 1 = single-kernel library call
        right in front of a weight gradient, 0 = other"""
        L = self.L
        single = (L.bn_act_bwd_apply, L.pw_bwd)
        n = len(self.bwd)
        roles = [2 if getattr(fn, "__name__", "") == "conv2d_wgrad" else 0 for fn, _ in self.bwd]
        if self.defer_slab_reduce:
            for i, (fn, _) in enumerate(self.bwd):
                info = getattr(fn, "info", None)
                if roles[i] == 2 and info is not None and len(info) > 7 and info[7] == 0:        # k == 0: the reduce alone (engine._emit_pw_bwd1)
                    roles[i] = 3
        if self.fork_on_dispatch:
            for i in range(n - 1):
                if roles[i] == 0 and roles[i + 1] == 2 and any(self.bwd[i][0] is f for f in single):
                    roles[i] = 1
        return roles

    def run_backward(self, gout):
        self.gscale.copy_(gout.reshape(-1)[:self.gscale.numel()], non_blocking=True)
        if self.use_graph:
            self._graphed("bwd")
        else:
            self.run_bwd_list()


class FlatParamsMixin:
    """Keeps all parameters (and their gradients) as views of two flat fp32 buffers so the optimizer step and the RCCL
    gradient all-reduce are single passes over contiguous HBM."""

    def _flatten(self):
        if getattr(self, "_pipe_plan", None) is not None:
            self._param_sync()                               # a pipelined optimizer step may still be updating the old buffers
        plist = [p for p in self.parameters()]
        dev = plist[0].device
        total = sum((p.numel() + 3) & ~3 for p in plist)           # every parameter starts on a 16-byte boundary (float4 rows in the pack kernel;
        pflat = torch.zeros(total, dtype=torch.float32, device=dev)  # the 255-element head biases would misalign everything behind them); padding stays 0
        gflat = torch.zeros(total, dtype=torch.float32, device=dev)
        off = 0
        self._goff = {}
        with torch.no_grad():
            for p in plist:
                n = p.numel()
                pflat[off:off + n].copy_(p.data.reshape(-1))
                p.data = pflat[off:off + n].view(p.shape)
                self._goff[id(p)] = (off, n)
                off += (n + 3) & ~3
        self._plist, self._pflat, self._gflat = plist, pflat, gflat
        self._flat_ptrs = [p.data_ptr() for p in plist]
        self._plans = {}
        self._pipe_plan = None
        self._last_train_plan = None         # it was built on the old flat buffers: a pipelined optimizer step must not reuse its pack table
        self._params_changed()

    # run-time caches that must not travel with a copy / pickle of the model: launch plans hold ctypes function pointers, raw device
    # pointers and closures (copy.deepcopy(model) after a forward -- RektNet/train_eval.py:99 -- raised "ctypes objects containing
    # pointers cannot be pickled"); the copy re-flattens its parameters and rebuilds its plans on first use.
    def _replicate_for_data_parallel(self):
        """nn.DataParallel (reference train.py:193-195 wraps the model when torch.cuda.device_count() > 1) copies the module tree onto
        every device per forward.  These models own flat parameter / gradient buffers, ctypes launch plans bound to raw device
        pointers, and side streams: a replica would launch kernels on device 0's memory.  Fail loudly instead."""
        raise RuntimeError(
            f"{type(self).__name__} cannot be replicated by torch.nn.DataParallel: the MI355X-native path is one process per GPU. "
            "Launch the script with `python -m torch.distributed.run --nproc-per-node N ...`, give every rank its shard of the batch and "
            "attach `mdcv.parallel.GradAllReducer.attach(model)` (all-reduce(SUM) of the flat gradient over RCCL -- the same per-shard "
            "BatchNorm / build_targets + summed-gradient semantics as DataParallel), or hide the other GPUs from a single-process run "
            "(HIP_VISIBLE_DEVICES=0).  See INTEGRATION.md §1.")

    _TRANSIENT = ("_plans", "_pipe_plan", "_last_train_plan", "_dp_reducer", "_dp_auto", "_pflat", "_gflat", "_flat_ptrs", "_goff", "_plist", "_flat_parent")

    def _state_without_plans(self):
        d = {k: v for k, v in self.__dict__.items() if k not in self._TRANSIENT}
        d["_plans"] = {}
        return d

    # Launch plans are cached per (batch shape, mode) and own every buffer they touch (~10 GB for YOLOv3 at batch 32), so the cache
    # is an LRU bounded by activation bytes (MDCV_PLAN_CACHE_GB, default 48) and by count (MDCV_MAX_PLANS, default 16): a ragged last
    # batch (the reference's DataLoader has no drop_last) or validation at other resolutions costs extra plans only while they are
    # in use, not one per shape ever seen.  The plan in use is never evicted.
    max_plans = int(os.environ.get("MDCV_MAX_PLANS", "16"))
    max_plan_bytes = int(float(os.environ.get("MDCV_PLAN_CACHE_GB", "48")) * (1 << 30))

    def _plan_lookup(self, key):
        plan = self._plans.get(key)
        if plan is not None and next(reversed(self._plans)) != key:
            self._plans[key] = self._plans.pop(key)          # most recently used last
        return plan

    def _plan_store(self, key, plan):
        self._plans[key] = plan
        while len(self._plans) > 1 and (len(self._plans) > max(1, self.max_plans) or
                                        sum(getattr(p, "bytes", 0) for p in self._plans.values()) > self.max_plan_bytes):
            victim = next(k for k in self._plans if k != key)
            self._evict_plan(victim)

    def _evict_plan(self, key):
        plan = self._plans.pop(key)
        try:
            if getattr(self, "_pipe_plan", None) is plan:
                self._param_sync()                           # its deferred parameter-group updates must land first
                self._pipe_plan = None
        finally:
            if getattr(self, "_last_train_plan", None) is plan:
                self._last_train_plan = None
        plan.check_targets()                                 # a pending bad-label flag must not be lost with the plan (last batch of a run);
                                                             # raised AFTER the bookkeeping above, so the model is consistent when it does
        # the plan's buffers go back to the caching allocator when the last reference dies (an autograd graph that still needs the
        # plan for its backward holds one); every stream that used them was joined into the current stream at the end of its step

    def release_plans(self):
        """Drop every cached launch plan (and its HBM buffers); the next forward rebuilds what it needs."""
        err = None
        for k in list(getattr(self, "_plans", {})):
            try:
                self._evict_plan(k)
            except IndexError as e:                          # a pending bad-label flag: drop every plan first, then report it
                err = e
        if err is not None:
            raise err

    def _params_changed(self):
        """Parameters were rewritten behind the optimizer's back (load_weights / load_state_dict): operands packed ahead of the next
        forward by a pipelined optimizer step are stale."""
        self._param_epoch = getattr(self, "_param_epoch", 0) + 1

    def _param_versions(self):
        """Sum of the parameters' autograd version counters: moves when user code edits any parameter in place (the HIP kernels do not)."""
        return sum(p._version for p in self._plist)

    def _flat_ok(self):
        pl = getattr(self, "_plist", None)
        if pl is None:
            return False
        return all(p.data_ptr() == q for p, q in zip(pl, self._flat_ptrs))       # every parameter still is its view of the flat buffer (~15 us)

    def _grad_view(self, p):
        off, n = self._goff[id(p)]
        return self._gflat[off:off + n].view(p.shape)

    def flat_parameters(self):
        """(flat fp32 parameter buffer, flat fp32 gradient buffer) — what FusedAdam / the all-reduce operate on."""
        if not self._flat_ok():
            self._flatten()
        self._param_sync()
        return self._pflat, self._gflat

    def _param_sync(self):
        """Orders the current stream behind a pipelined optimizer step (optim.py, pipeline=True) that may still be updating
        parameter groups on the parameter stream.  Every reader of the parameters outside the pipelined forward goes through here."""
        plan = getattr(self, "_pipe_plan", None)
        if plan is None:
            return
        for k in range(len(plan._pending_updates)):
            plan.launch_param_group(k, gated=False)
        for k, ev in enumerate(plan._group_events):
            if ev is not None:
                torch.cuda.current_stream().wait_event(ev)
                plan._group_events[k] = None

    _dp_average = False                                      # KeypointNet overrides: its loss is a batch MEAN (see rektnet/keypoint_net.py)

    def _auto_dp_shard(self, *tensors):
        """Under torchrun with the drop-in modules (parallel.enable_auto_data_parallel): rank r's share of a training batch -- nn.DataParallel's
        scatter on dim 0, reference train.py:68 / :193-195 -- and, on first use, the overlapped gradient all-reduce attached to this model and
        the replicas synchronised from rank 0.  -> (tensors, weight): weight 0.0 marks a rank whose chunk was empty (its outputs are to be
        multiplied by zero), None / 1.0 anything else.  Off (the usual case): the tensors pass through."""
        from .parallel import auto_shard, auto_attach
        out, weight = auto_shard(*tensors)
        if weight is not None:
            auto_attach(self, average=self._dp_average)
        return out, weight

    def _run_backward(self, plan, gout):
        self._last_train_plan = plan
        pl = self._plist
        keep = None
        if pl[0].grad is not None:                       # gradients were not reset to None: accumulate semantics
            keep = self._gflat.clone()
        red = getattr(self, "_dp_reducer", None)
        # (an attached reducer with ONE rank has nothing to exchange: no markers, and the backward keeps its single-GPU schedule -- the markers switch
        #  off the deferred slab reduces of run_bwd_list, 32 forks = 0.17 ms of main queue per YOLOv3 step, which bench.py at --gpus 1 paid until round 5)
        overlap = red is not None and red._active() and keep is None and not plan.use_graph
        plan.on_ready = red.on_ready if overlap else None
        if red is not None:
            red.extra_streams = [plan.side()] if (plan.overlap_wgrad and not plan.use_graph and self._gflat.is_cuda) else []
            red.begin(self._gflat, overlap)
        plan.run_backward(gout)
        plan.on_ready = None
        if keep is not None:
            self._gflat.add_(keep)
        if red is not None:
            red.backward_done()
            if getattr(self, "_dp_auto", False):
                red.finish()                                 # (auto data parallel: nobody else will order the optimizer behind the exchange)
        for p in pl:
            v = self._grad_view(p)
            if p.grad is None:
                p.grad = v
            elif p.grad.data_ptr() != v.data_ptr():      # foreign .grad tensor: fold ours in, then re-point
                v.add_(p.grad)
                p.grad = v
        # a label with cx / cy >= 1.0 (reference: IndexError inside build_targets, BEFORE any update, utils/utils.py:262).  Looked at HERE, with
        # the backward launches already queued: the host's wait for the flag copy behind the forward then costs the GPU nothing (at the head
        # of the backward it left the GPU idle until the first backward launch arrived: 13.77 vs 13.65 ms per step), the heads dropped the
        # bad target in the forward so the queued backward is well defined, and the error still leaves backward() -- before optimizer.step()
        plan.check_targets(block=getattr(self, "strict_targets", True))



def _sync_before_state_dict(module, prefix, keep_vars):
    module._param_sync()


def _zero_tensor(t, stream):
    t.zero_()
    return 0


def _bump_counters(ts, stream):
    torch._foreach_add_(ts, 1)
    return 0
