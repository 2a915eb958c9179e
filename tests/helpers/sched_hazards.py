"""Launch-schedule hazards of a training step, proved on the host from what a real step enqueued.

A training step is not one queue: weight gradients run on a side stream (netplan._NetPlan.run_bwd_list: mdcv_stream_fork, fork-on-dispatch
with mdcv_stream_fork_arm / _wait, deferred slab reduces), a pipelined FusedAdam updates and re-packs parameter groups on a third stream behind
torch events.  This helper has three parts:

  Recorder   a stand-in for the object `mdcv._lib.lib()` returns.  It forwards every call to the real library, returns its result, and appends
             (entry name, args, stream handle) to a trace; mdcv_stream_fork / _arm / _wait become synchronisation records.  While a recording
             is open it also wraps torch.cuda.Stream.wait_stream / wait_event / record_event and torch.cuda.Event.record (log, then forward).
             Torch-side work (copies, memsets, counters) is invisible to it and is entered BY NAME from TORCH_ENTRIES as an access on torch's
             current stream; a launch-list entry that makes no library call and has no row there is reported, never skipped.
  TABLE      per entry point, the bytes each pointer argument covers, as strided sets (ptr, rows, row pitch, bytes used per row).  The DIRECTION is
             not in the table: it comes from include/mdcv_hip.h (`const T*` = read, anything else = read + write unless the row says write-only).
  analyse()  vector clocks over streams; the result is every pair of launches that touch the same bytes, at least one writing, whose later
             launch is not ordered behind the earlier one by the synchronisation that was actually enqueued.

What the model is, and what it takes as given:

  * A stream is an in-order queue.  The null stream (handle 0) is treated as ONE MORE such queue with no implicit ordering against the others:
    every other stream of a step is non-blocking -- engine.checked_stream / side_stream and the optimizer's parameter stream are
    torch.cuda.Stream(device=...) objects, which torch takes from its stream pool, and the pool's streams are created with
    hipStreamNonBlocking (c10/hip HIPStream.cpp: hipStreamCreateWithPriority(..., hipStreamNonBlocking, ...)) -- so the legacy stream's implicit
    barrier does not exist for them and nothing may rely on it.
  * stream_fork(from, to): everything recorded on `from` so far happens before what is recorded on `to` afterwards.  wait_stream the same.
    Event.record(s) snapshots the clock of s; wait_event merges the snapshot of the record that PRECEDED it in enqueue order (HIP semantics
    of a re-recorded event).  stream_fork_arm(from) binds its event to the NEXT recorded library call of the thread; the snapshot is `from`'s
    clock including that call; stream_fork_wait(to, ev) merges it.  Reported as model violations: the next call is on another stream than
    `from`; a wait before any call; a wait on an event never recorded.
  * GIVEN (1): the armed call launches exactly ONE kernel.  csrc/common.h MDCV_LAUNCH hands the armed event to the first kernel the thread
    launches, so a two-kernel call would release the side stream one kernel early.  tests/test_gpu_sched_hazards.py checks the kernel count of
    every armed entry in a pass of its own (profiling changes the arm path, so it cannot be the recorded pass).
  * GIVEN (2): HIP's documented semantics of the stop event of hipExtLaunchKernelGGL -- it is recorded when that dispatch has completed, and a
    hipStreamWaitEvent on it orders later work of the waiting stream behind the dispatch (and, the queue being in order, behind everything in
    front of it on its stream).
  * The `device_scope` flag of the forks is about VISIBILITY (which cache level the release reaches), not order.  It is not modelled.
  * Extents are hulls of what a kernel may touch.  Two strided sets of one pitch inside one allocation overlap only if their byte columns
    overlap (channel slices of one NHWC buffer: concat targets, Act.slice); anything else is compared by hull.
  * mdcv_bn_stats_finalize / mdcv_bn_bwd_finalize_rows fold more than 4096 partial rows in place: their `partial` is not `const` in the header,
    so it is a read + write here like any other scratch, and the analysis orders it itself.
  * No extent in TABLE runs "to the end of the containing allocation": every one is computed from the call's arguments or a size query.
  * One thread.  The library keeps the armed event per thread (`thread_local`, csrc/common.h) and the recorder keeps no thread id: "the next
    recorded library call" is the next call of ANY thread.  run_bwd_list arms and launches back to back on one thread, and the steps recorded
    here run on one thread; a multi-threaded driver would need the thread in every record.

Out of scope: data-parallel runs (the reducer's comm stream needs several processes), hipGraph mode (a captured list runs on one stream), the
loaders' staging streams.
"""
import bisect
import os
import re
import struct
import types

F32, BF16 = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HEADER = os.path.join(ROOT, "include", "mdcv_hip.h")


# ------------------------------------------------------------------------------------------------ header: directions
def parse_directions(path=HEADER):
    """-> {entry (without mdcv_): [(arg name, is pointer, is const)]} for every prototype; `const` is kept (mdcv._lib.parse_header drops it)"""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(int|long long)\s+mdcv_(\w+)\s*\(([^)]*)\)\s*;", text):
        args = []
        for a in (x.strip() for x in m.group(3).split(",")):
            if not a or a == "void":
                continue
            name = re.split(r"[\s\*]+", a)[-1]
            args.append((name, "*" in a, bool(re.match(r"const\b", a))))
        out[m.group(2)] = args
    return out


def stream_entries(directions):
    return sorted(n for n, args in directions.items() if any(a[0] == "stream" for a in args))


# ------------------------------------------------------------------------------------------------ strided sets
def flat(p, nbytes):
    """a contiguous range"""
    return None if not p or nbytes <= 0 else (int(p), 1, int(nbytes), int(nbytes))


def rows(p, M, ld, C, es):
    """M rows of C elements, `ld` elements apart (an NHWC activation view)"""
    return None if not p or M <= 0 or C <= 0 else (int(p), int(M), int(ld) * es, int(C) * es)


def hull(s):
    p, r, pitch, used = s
    return p, p + (r - 1) * pitch + used


def overlap(a, b, base=0):
    """(lo, hi) of the bytes two strided sets may share, or None.  Same pitch (a single row takes the other's): disjoint byte columns do not
    overlap; otherwise the hulls decide."""
    (alo, ahi), (blo, bhi) = hull(a), hull(b)
    lo, hi = max(alo, blo), min(ahi, bhi)
    if lo >= hi:
        return None
    pa = a[2] if a[1] > 1 else (b[2] if b[1] > 1 else 0)
    pb = b[2] if b[1] > 1 else pa
    if pa and pa == pb:
        ca, cb = (a[0] - base) % pa, (b[0] - base) % pa
        if ca + a[3] <= pa and cb + b[3] <= pa and (ca + a[3] <= cb or cb + b[3] <= ca):
            return None
    return lo, hi


# ------------------------------------------------------------------------------------------------ the extent table
def E(dt):
    return 2 if (int(dt) & 0xff) == BF16 else 4


def _vec(name, count):
    return lambda a, q: flat(a[name], 4 * a[count])


def _act(ptr, M, ld, C, es=lambda a: E(a["dtype"])):
    return lambda a, q: rows(a[ptr], M(a), a[ld], a[C] if isinstance(C, str) else C(a), es(a))


_pin = lambda a: a["B"] * a["Hin"] * a["Win"]        # noqa: E731
_pout = lambda a: a["B"] * a["Hout"] * a["Wout"]     # noqa: E731
_bhw = lambda a: a["B"] * a["H"] * a["W"]            # noqa: E731
_M = lambda a: a["M"]                                # noqa: E731


def _conv_ws(a, q):
    return flat(a["ws"], 4 * a["splits"] * a["Cout"] * a["KH"] * a["KW"] * a["Cin"])


def _conv_common():
    return {"in": _act("in", _pin, "in_ldc", "Cin"), "out": _act("out", _pout, "out_ldc", "Nout"),
            "w_packed": lambda a, q: flat(a["w_packed"], E(a["dtype"]) * a["Nout"] * a["KH"] * a["KW"] * a["Cin"])}


def _pool_out(a):
    if "k" in a:
        return a["B"] * ((a["H"] + 2 * a["pad"] - a["k"]) // a["stride"] + 1) * ((a["W"] + 2 * a["pad"] - a["k"]) // a["stride"] + 1)
    return a["B"] * (a["H"] // a["stride"]) * (a["W"] // a["stride"]) if a["stride"] == 2 else _bhw(a)


def _pack_rows(a, q):
    """the 72-byte records of engine.Plan.finish_pack: the launch reads every listed weight (and bias) and writes every listed wf / wd / bias_pad"""
    es = E(a["dtype"])
    out = []
    raw = q.read(a["table"], 72 * a["nlayers"])
    for i in range(a["nlayers"]):
        w, wf, wd, cout, cin, kk, cop, cip, _, _, _, b, bp = struct.unpack_from("<QQQiiiiiiiiQQ", raw, 72 * i)
        out.append((f"table[{i}].w_oihw", "r", flat(w, 4 * cout * cin * kk)))
        out.append((f"table[{i}].w_fwd", "w", flat(wf, es * cop * kk * cip)))
        out.append((f"table[{i}].w_dgrad", "w", flat(wd, es * cop * kk * cip)))
        out.append((f"table[{i}].bias", "r", flat(b, 4 * cout)))
        out.append((f"table[{i}].bias_padded", "w", flat(bp, 4 * cop) if b else None))
    return out


def _ema_segments(a, q):
    out = []
    raw = q.read(a["table"], 24 * a["n_segments"])
    for i in range(a["n_segments"]):
        src, off, ln = struct.unpack_from("<Qqq", raw, 24 * i)
        if src and 0 <= off and off + ln <= a["ema_elems"]:
            out.append((f"table[{i}].src", "r", flat(src, 4 * ln)))
            out.append((f"ema[{off}:{off + ln}]", "rw", flat(a["ema"] + 4 * off, 4 * ln)))
    return out


def _nbn(a):
    return 3 if a["y2"] else 2


_C = lambda n: _vec(n, "C")          # noqa: E731
_N = lambda n: _vec(n, "Nout")       # noqa: E731

# entry -> {"ptrs": {pointer argument: (args, queries) -> strided set | None}, "wo": write-only pointers, "indirect": (args, queries) ->
# [(label, "r" | "w" | "rw", set)] for memory reached through a device table}
TABLE = {
    "conv2d": dict(ptrs={**_conv_common(), "bias": _N("bias"), "addsrc": _act("addsrc", _pout, "add_ldc", "Nout"),
                         "stats_partial": lambda a, q: flat(a["stats_partial"], 8 * a["Nout"] * q.L.conv2d_stats_rows_geom(
                             a["dtype"], a["B"], a["Hout"], a["Wout"], a["Cin"], a["Nout"], a["KH"], a["KW"], a["stride"], a["pad"], a["dil"],
                             a["in_ldc"]))},
                   wo={"out", "stats_partial"}),
    "conv2d_xstats": dict(ptrs={**_conv_common(), "bias": _N("bias"),
                                "xacc": lambda a, q: flat(a["xacc"], 8 * q.L.xstats_words(a["reps"], a["Nout"]))}, wo={"out"}),
    "conv2d_dgrad_bnsums": dict(ptrs={**_conv_common(), "addsrc": _act("addsrc", _pout, "add_ldc", "Nout"), "y": _act("y", _pout, "ldy", "Nout"),
                                      "scale": _N("scale"), "shift": _N("shift"), "mean": _N("mean"),
                                      "partial": lambda a, q: flat(a["partial"], 8 * a["Nout"] * q.L.conv2d_dgrad_bnsums_rows(
                                          a["dtype"], a["B"], a["Hin"], a["Win"], a["Cin"], a["Hout"], a["Wout"], a["Nout"], a["KH"], a["KW"],
                                          a["stride"], a["pad"], a["dil"], a["in_ldc"]))},
                                wo={"out", "partial"}),
    "first_conv_stats": dict(ptrs={"x": _act("x", _bhw, "ldx", lambda a: 8), "w_packed": lambda a, q: flat(a["w_packed"], E(a["dtype"]) * 32 * 9 * 8),
                                   "partial": lambda a, q: flat(a["partial"], 4 * 2 * 32 * q.L.first_conv_rows(a["B"], a["H"]))}, wo={"partial"}),
    "first_conv_bn_act": dict(ptrs={"x": _act("x", _bhw, "ldx", lambda a: 8), "w_packed": lambda a, q: flat(a["w_packed"], E(a["dtype"]) * 32 * 9 * 8),
                                    "scale": lambda a, q: flat(a["scale"], 128), "shift": lambda a, q: flat(a["shift"], 128),
                                    "y": _act("y", _bhw, "ldy", lambda a: 32), "z": _act("z", _bhw, "ldz", lambda a: 32)}, wo={"y", "z"}),
    "pw_conv_fwd": dict(ptrs={"y": _act("y", _M, "ldy", "K"), "scale": _vec("scale", "K"), "shift": _vec("shift", "K"),
                              "resid": _act("resid", _M, "ldr", "K"), "z_out": _act("z_out", _M, "ldz", "K"),
                              "w_packed": lambda a, q: flat(a["w_packed"], E(a["dtype"]) * a["N"] * a["K"]), "bias": _vec("bias", "N"),
                              "out": _act("out", _M, "out_ldc", "N"),
                              "stats_partial": lambda a, q: flat(a["stats_partial"], 8 * a["N"] * q.L.pw_rows(a["M"], a["K"]))},
                        wo={"z_out", "out", "stats_partial"}),
    "pw_conv_fwd_xstats": dict(ptrs={"y": _act("y", _M, "ldy", "K"), "scale": _vec("scale", "K"), "shift": _vec("shift", "K"),
                                     "resid": _act("resid", _M, "ldr", "K"), "z_out": _act("z_out", _M, "ldz", "K"),
                                     "w_packed": lambda a, q: flat(a["w_packed"], E(a["dtype"]) * a["N"] * a["K"]), "bias": _vec("bias", "N"),
                                     "out": _act("out", _M, "out_ldc", "N"),
                                     "xacc": lambda a, q: flat(a["xacc"], 8 * q.L.xstats_words(a["reps"], a["N"]))}, wo={"z_out", "out"}),
    "bn_act_fwd_xstats": dict(ptrs={"y": _act("y", _M, "ldy", "C"), "xacc": lambda a, q: flat(a["xacc"], 8 * q.L.xstats_words(a["reps"], a["C"])),
                                    "gamma": _C("gamma"), "beta": _C("beta"), "running_mean": _C("running_mean"), "running_var": _C("running_var"),
                                    "scale": _C("scale"), "shift": _C("shift"), "mean": _C("mean"), "invstd": _C("invstd"),
                                    "resid": _act("resid", _M, "ldr", "C"), "out": _act("out", _M, "ldo", "C")},
                              wo={"scale", "shift", "mean", "invstd", "out"}),
    "bn_act_fwd": dict(ptrs={"y1": _act("y1", _M, "ld1", "C"), "s1": _C("s1"), "b1": _C("b1"), "y2": _act("y2", _M, "ld2", "C"), "s2": _C("s2"),
                             "b2": _C("b2"), "resid": _act("resid", _M, "ldr", "C"), "out": _act("out", _M, "ldo", "C")}, wo={"out"}),
    "bn_stats_finalize": dict(ptrs={"partial": lambda a, q: flat(a["partial"], 8 * a["C"] * a["rows"]), "accum": lambda a, q: flat(a["accum"], 24 * a["C"]),
                                    "gamma": _C("gamma"), "beta": _C("beta"), "running_mean": _C("running_mean"), "running_var": _C("running_var"),
                                    "scale": _C("scale"), "shift": _C("shift"), "mean": _C("mean"), "invstd": _C("invstd")},
                              wo={"scale", "shift", "mean", "invstd"}),
    "bn_act_bwd_reduce_finalize": dict(ptrs={
        "dout": _act("dout", _M, "ldd", "C"), "y1": _act("y1", _M, "ld1", "C"), "y2": _act("y2", _M, "ld2", "C"),
        **{n: _C(n) for n in ("s1", "b1", "mean1", "invstd1", "s2", "b2", "mean2", "invstd2", "gamma1", "dgamma1", "dbeta1", "cA1", "cB1", "cC1",
                              "gamma2", "dgamma2", "dbeta2", "cA2", "cB2", "cC2")},
        "partial_ws": lambda a, q: flat(a["partial_ws"], 4 * q.L.bn_act_bwd_reduce_ws_floats(a["dtype"], a["M"], a["C"], _nbn(a)))},
        wo={"dgamma1", "dbeta1", "cA1", "cB1", "cC1", "dgamma2", "dbeta2", "cA2", "cB2", "cC2"}),
    "bn_bwd_finalize_rows": dict(ptrs={"partial": lambda a, q: flat(a["partial"], 8 * a["C"] * a["rows"]),
                                       **{n: _C(n) for n in ("gamma", "mean", "invstd", "dgamma", "dbeta", "cA", "cB", "cC")}},
                                 wo={"dgamma", "dbeta", "cA", "cB", "cC"}),
    "bn_act_bwd_apply": dict(ptrs={"dout": _act("dout", _M, "ldd", "C"), "y1": _act("y1", _M, "ld1", "C"), "y2": _act("y2", _M, "ld2", "C"),
                                   "dy1": _act("dy1", _M, "ldy1", "C"), "dy2": _act("dy2", _M, "ldy2", "C"),
                                   **{n: _C(n) for n in ("s1", "b1", "cA1", "cB1", "cC1", "s2", "b2", "cA2", "cB2", "cC2")}}, wo={"dy1", "dy2"}),
    "colsum_f32": dict(ptrs={"x": _act("x", _M, "ldc", "C"), "out": _C("out"),
                             "partial_ws": lambda a, q: flat(a["partial_ws"], 4 * q.L.colsum_ws_floats(a["dtype"], a["M"], a["C"]))}, wo={"out"}),
    "conv2d_wgrad": dict(ptrs={"dy": _act("dy", _pout, "dy_ldc", "Cout"), "x": _act("x", _pin, "x_ldc", "Cin"), "ws": _conv_ws,
                               "dw_oihw": lambda a, q: flat(a["dw_oihw"], 4 * a["Cout_real"] * a["Cin_real"] * a["KH"] * a["KW"])}, wo={"ws"}),
    "conv2d_wgrad_bnapply": dict(ptrs={"dz": _act("dz", _pout, "dz_ldc", "Cout"), "y": _act("y", _pout, "y_ldc", "Cout"),
                                       **{n: _vec(n, "Cout") for n in ("scale", "shift", "cA", "cB", "cC")}, "x": _act("x", _pin, "x_ldc", "Cin"),
                                       "ws": _conv_ws,
                                       "dw_oihw": lambda a, q: flat(a["dw_oihw"], 4 * a["Cout_real"] * a["Cin_real"] * a["KH"] * a["KW"])}, wo={"ws"}),
    "wgrad_reduce": dict(ptrs={"ws": lambda a, q: flat(a["ws"], 4 * a["splits"] * a["Cout_pad"] * a["KK"] * a["Cin_pad"]),
                               "dw_oihw": lambda a, q: flat(a["dw_oihw"], 4 * a["Cout"] * a["Cin"] * a["KK"])}),
    "pw_bwd": dict(ptrs={"dy": _act("dy", _M, "ldy", "Cout"), "x": _act("x", _M, "ldx", "Cin"),
                         "wd_packed": lambda a, q: flat(a["wd_packed"], E(a["dtype"]) * a["Cin"] * a["Cout"]), "dx": _act("dx", _M, "lddx", "Cin"),
                         "addsrc": _act("addsrc", _M, "ldadd", "Cin"), "ws": lambda a, q: flat(a["ws"], 4 * a["slabs"] * a["Cout"] * a["Cin"]),
                         "fy": _act("fy", _M, "ldfy", "Cin"), "fscale": _vec("fscale", "Cin"), "fshift": _vec("fshift", "Cin"),
                         "fmean": _vec("fmean", "Cin"), "fpartial": lambda a, q: flat(a["fpartial"], 8 * a["slabs"] * a["Cin"])},
                   wo={"dx", "ws", "fpartial"}),
    "pack_weights_batched": dict(ptrs={"table": lambda a, q: flat(a["table"], 72 * a["nlayers"])}, indirect=_pack_rows),
    "nchw_to_nhwc": dict(ptrs={"src": lambda a, q: flat(a["src"], 4 * a["B"] * a["C"] * a["H"] * a["W"]), "dst": _act("dst", _bhw, "ldc", "Cpad")},
                         wo={"dst"}),
    "upsample2x_fwd": dict(ptrs={"in": _act("in", _bhw, "ldi", "C"), "out": _act("out", lambda a: 4 * _bhw(a), "ldo", "C")}, wo={"out"}),
    "upsample2x_bwd": dict(ptrs={"dout": _act("dout", lambda a: 4 * _bhw(a), "ldo", "C"), "din": _act("din", _bhw, "ldi", "C")}, wo={"din"}),
    "upsample_fwd": dict(ptrs={"in": _act("in", _bhw, "ldi", "C"), "out": _act("out", lambda a: a["scale"] ** 2 * _bhw(a), "ldo", "C")}, wo={"out"}),
    "upsample_bwd": dict(ptrs={"dout": _act("dout", lambda a: a["scale"] ** 2 * _bhw(a), "ldo", "C"), "din": _act("din", _bhw, "ldi", "C")}, wo={"din"}),
    **{n: dict(ptrs={"in": _act("in", _bhw, "ldi", "C"), "out": _act("out", _pool_out, "ldo", "C"),
                     "idx": lambda a, q: flat(a["idx"], _pool_out(a) * a["C"])}, wo={"out", "idx"}) for n in ("maxpool2x2_fwd", "maxpool_fwd")},
    **{n: dict(ptrs={"dout": _act("dout", _pool_out, "ldo", "C"), "idx": lambda a, q: flat(a["idx"], _pool_out(a) * a["C"]),
                     "din": _act("din", _bhw, "ldi", "C")}, wo={"din"}) for n in ("maxpool2x2_bwd", "maxpool_bwd")},
    **{n: dict(ptrs={"logits": _act("logits", lambda a: a["B"] * a["Gh"] * a["Gw"], "ldc", "Cpad"),
                     "dlogits": _act("dlogits", lambda a: a["B"] * a["Gh"] * a["Gw"], "ldd", "Cpad"),
                     "targets": lambda a, q: flat(a["targets"], 20 * a["B"] * a["T"]), "anchors_scaled": lambda a, q: flat(a["anchors_scaled"], 8 * a["A"]),
                     "workspace": lambda a, q: flat(a["workspace"], q.L.yolo_head_workspace_bytes(a["B"], a["A"], a["Gh"], a["Gw"])),
                     "gscale": lambda a, q: flat(a["gscale"], 4), **({"out7": lambda a, q: flat(a["out7"], 28)} if n == "yolo_head_train" else {})},
               wo={"dlogits"}) for n in ("yolo_head_train", "yolo_head_grad")},
    "head1x1_f32": dict(ptrs={"x_bf16": lambda a, q: rows(a["x_bf16"], a["M"], a["ldx"], a["C"], 2), "w": lambda a, q: flat(a["w"], 4 * a["K"] * a["C"]),
                              "bias": _vec("bias", "K"), "out": lambda a, q: flat(a["out"], 32 * a["M"])}, wo={"out"}),
    "softargmax_fwd": dict(ptrs={"logits": _act("logits", _bhw, "ldc", "K"), "hm": lambda a, q: flat(a["hm"], 4 * a["K"] * _bhw(a)),
                                 "pts": lambda a, q: flat(a["pts"], 8 * a["B"] * a["K"])}, wo={"hm", "pts"}),
    "softargmax_bwd": dict(ptrs={"hm": lambda a, q: flat(a["hm"], 4 * a["K"] * _bhw(a)), "pts": lambda a, q: flat(a["pts"], 8 * a["B"] * a["K"]),
                                 "dpts": lambda a, q: flat(a["dpts"], 8 * a["B"] * a["K"]), "dhm": lambda a, q: flat(a["dhm"], 4 * a["K"] * _bhw(a)),
                                 "sdot_ws": lambda a, q: flat(a["sdot_ws"], 4 * a["B"] * a["K"]),
                                 "dlogits": _act("dlogits", _bhw, "ldd", lambda a: (a["K"] + 7) // 8 * 8)}, wo={"dlogits"}),
    "adam_step": dict(ptrs={n: (lambda a, q, n=n: flat(a[n], 4 * a["n"])) for n in ("params", "grads", "exp_avg", "exp_avg_sq")}),
    "adam_step_guarded": dict(ptrs={**{n: (lambda a, q, n=n: flat(a[n], 4 * a["n"])) for n in ("params", "grads", "exp_avg", "exp_avg_sq")},
                                    "block": lambda a, q: flat(a["block"], 72)}),
    "sgd_step": dict(ptrs={n: (lambda a, q, n=n: flat(a[n], 4 * a["n"])) for n in ("params", "grads", "momentum_buf")}),
    "sgd_step_guarded": dict(ptrs={**{n: (lambda a, q, n=n: flat(a[n], 4 * a["n"])) for n in ("params", "grads", "momentum_buf")},
                                   "block": lambda a, q: flat(a["block"], 72)}),
    "grad_sumsq": dict(ptrs={"grads": lambda a, q: flat(a["grads"], 4 * a["n"]), "partials": lambda a, q: flat(a["partials"], 8 * ((a["n"] + 4095) // 4096))},
                       wo={"partials"}),
    "grad_guard_finalize": dict(ptrs={"partials": lambda a, q: flat(a["partials"], 8 * a["n_partials"]), "block": lambda a, q: flat(a["block"], 72),
                                      "history": lambda a, q: flat(a["history"], 4 * a["ring"])}),
    "ema_advance": dict(ptrs={"block": lambda a, q: flat(a["block"], 24), "guard": lambda a, q: flat(a["guard"], 72)}),
    "ema_update": dict(ptrs={"ema": lambda a, q: flat(a["ema"], 4 * a["n"]), "params": lambda a, q: flat(a["params"], 4 * a["n"]),
                             "block": lambda a, q: flat(a["block"], 24)}),
    # the `ema` argument is only the base of the segments: what the launch touches of it is listed row by row through `indirect`
    "ema_update_segments": dict(ptrs={"ema": lambda a, q: None, "table": lambda a, q: flat(a["table"], 24 * a["n_segments"]),
                                      "block": lambda a, q: flat(a["block"], 24)}, indirect=_ema_segments),
}

_INFER = "inference plans only: no training step launches it"
_DATA = "data loading / augmentation: runs on the loaders' staging path, outside the training step (out of scope)"
_POST = "detection / key-point post-processing and evaluation: never part of a training step"
_OLD = "two-stage form kept for callers outside the plans; the plans use the one-launch form"
_RT = "runtime plumbing (events, graphs, probes, RCCL): launches no kernel of a plan; hipGraph and data-parallel runs are out of scope"
NOT_IN_PLANS = {
    "conv2d_affine_act": _INFER, "bn_eval_coeffs": _INFER, "bn_eval_coeffs_bias": _INFER, "yolo_head_decode": _INFER, "nhwc_to_nchw": _INFER,
    "pack_weights": "single-layer form; the plans pack through the table-driven mdcv_pack_weights_batched",
    "partial_reduce": _OLD, "bn_finalize": _OLD, "bn_act_bwd_reduce": _OLD, "bn_bwd_finalize": _OLD, "colsum": _OLD, "accum_to_f32": _OLD,
    "bbox_iou": _POST, "build_targets": "stand-alone build_targets; the plans use the fused head (mdcv_yolo_head_train)",
    "cross_ratio_loss": "the loss module's own launch on tensors of the caller, outside the model's plan; the driver of these tests feeds dpts directly",
    "kpt_eval_rows": _POST, "nms": _POST, "detect_post": _POST, "average_precision": _POST, "crop_resize": _POST, "crop_resize_u8": _POST,
    "synth_cone_batch": _DATA, "synth_crop_batch": _DATA, "imgload_batch": _DATA, "imgload_aug_batch": _DATA, "imgload_frames_batch": _DATA,
    "imgload_aug_frames_batch": _DATA, "imgfx_batch": _DATA, "kptload_batch": _DATA,
    "detect_draw_boxes": _POST, "detect_map_boxes": _POST, "detect_merge_tiles": _POST, "crop_resize_frames_u8": _POST, "kpt_draw_points": _POST,
    "kpt_heatmap_mosaic": _POST, "detmap_match": _POST, "detmap_finalize": _POST, "kmeans_begin": _DATA, "kmeans_steps": _DATA,
    "ema_swap": "validation / checkpoint time (WeightEMA.applied), between steps on the current stream, behind _param_sync",
    "ema_swap_segments": "validation / checkpoint time (WeightEMA.applied), between steps on the current stream, behind _param_sync",
    "train_log_step": "the training loops' bookkeeping launch on the caller's tensors, outside the model's plan",
    "event_record": _RT, "probe_mfma": _RT, "graph_begin": _RT, "graph_end": _RT, "graph_launch": _RT, "comm_allreduce_sum": _RT,
}

SYNC_ENTRIES = ("stream_fork", "stream_fork_arm", "stream_fork_wait")

# torch-side launch-list entries, by name: (entry, args) -> [(label, mode, tensor)].  They run on torch's current stream.
TORCH_ENTRIES = {
    "copy_bias_grad": lambda fn, args: [("gb", "w", fn.__defaults__[0]), ("tmp", "r", fn.__defaults__[1])],    # gb.copy_(tmp[:n])
    "grad_ready": lambda fn, args: [],                       # a marker for the data-parallel reducer (none attached: nothing is enqueued)
    "wait_params": lambda fn, args: [],                      # only waits and launches of parameter groups, which are recorded themselves
    "_zero_tensor": lambda fn, args: [("t", "w", args[0])],  # t.zero_()
    "_bump_counters": lambda fn, args: [(f"ts[{i}]", "rw", t) for i, t in enumerate(args[0])],     # torch._foreach_add_(ts, 1)
    "mdcv_pack_weights_batched": lambda fn, args: [],        # pack_all's early return: the optimizer packed ahead, nothing is enqueued
}


# torch ops around the launch lists -- netplan.run_forward / run_backward, the autograd functions of the models, the label-flag copy of the
# Darknet plan -- which the step of the test driver runs on torch's current stream: name -> plan -> [(label, mode, tensor)].  (The accumulate
# path of FlatParamsMixin._run_backward, `_gflat.clone()` / `_gflat.add_`, is not exercised: the driver resets gradients to None.)
def _present(plan, mode, *names):
    return [(k, mode, getattr(plan, k)) for k in names if getattr(plan, k, None) is not None]


DRIVER_OPS = {
    "run_forward: targets.copy_": lambda plan: _present(plan, "w", "targets"),
    "after the forward: out7.clone() / hm.clone(), pts.clone(); cat(err_views) -> pinned host word":
        lambda plan: _present(plan, "r", "out7", "hm", "pts") + [(f"err_views[{i}]", "r", v) for i, v in enumerate(getattr(plan, "err_views", ()))],
    "run_backward: gscale.copy_ / dpts.copy_, dhm.copy_": lambda plan: _present(plan, "w", "gscale", "dpts", "_dhm"),
}


def form_of(name, a):
    """what distinguishes the code paths of one entry point: its switches and which optional pointers are given"""
    keys = ("dtype", "mode", "KH", "KW", "stride", "act", "fact", "accumulate", "k", "scale")
    return (name,) + tuple((k, a[k]) for k in keys if k in a and not isinstance(a[k], float)) + tuple(k for k, v in a.items() if v is None)


class Queries:
    """what the extent rows may ask: the library's own size queries (`L`) and the bytes of a device table (`read`)"""

    def __init__(self, L, read):
        self.L, self.read = L, read


def named_args(directions, name, args):
    """{argument name: value} of one recorded call; pointers as int or None"""
    spec = directions[name]
    out = {}
    for (n, is_ptr, _), v in zip(spec, args):
        if is_ptr:
            v = getattr(v, "value", v)
            v = int(v) if v else None
        out[n] = v
    return out


def accesses_of(directions, name, args, q):
    """[(label, ptr, rows, pitch, used, mode)] of one recorded library call, or raises KeyError for an entry without a row"""
    row = TABLE[name]
    a = named_args(directions, name, args)
    out = []
    for n, is_ptr, const in directions[name]:
        if not is_ptr or n == "stream" or a[n] is None:
            continue
        s = row["ptrs"][n](a, q)
        if s is not None:
            out.append((n, *s, "r" if const else ("w" if n in row.get("wo", ()) else "rw")))
    if "indirect" in row:
        out += [(lab, *s, mode) for lab, mode, s in row["indirect"](a, q) if s is not None]
    return out


# ------------------------------------------------------------------------------------------------ allocations
class Allocations:
    """the known allocations of a step: every device tensor reachable from the roots given (model with its plans, flat buffers and BatchNorm
    statistics; optimizer with moments, guard and EMA; the driver's inputs), by storage.  A pointer outside all of them does not resolve."""

    def __init__(self):
        self.by_base = {}
        self._sorted = None

    def add(self, name, base, size, tensor=None):
        if size > 0 and base not in self.by_base:
            self.by_base[base] = (name, base, size, tensor)
            self._sorted = None

    def collect(self, obj, name, seen=None, depth=0):
        import torch
        seen = {} if seen is None else seen                # id -> object (kept alive: an id must stay its object's)
        if id(obj) in seen or depth > 14 or obj is None:
            return
        if isinstance(obj, (str, bytes, int, float, bool, type, types.ModuleType, torch.cuda.Stream, torch.cuda.Event, torch.dtype, torch.device,
                            Recorder, _Logged)) or type(obj).__module__.split(".")[0] in ("ctypes", "_ctypes", "numpy", "weakref"):
            return
        seen[id(obj)] = obj
        if isinstance(obj, torch.Tensor):
            if obj.is_cuda:
                st = obj.untyped_storage()
                self.add(name, st.data_ptr(), st.nbytes(), obj)
            return
        if isinstance(obj, dict):
            for i, (k, v) in enumerate(obj.items()):
                self.collect(v, f"{name}[{k if isinstance(k, (str, int)) else i}]", seen, depth + 1)
            return
        if isinstance(obj, (list, tuple, set)):
            for i, v in enumerate(obj):
                self.collect(v, f"{name}[{i}]", seen, depth + 1)
            return
        if isinstance(obj, (types.FunctionType, types.MethodType)):
            f = getattr(obj, "__func__", obj)
            for i, v in enumerate(f.__defaults__ or ()):
                self.collect(v, f"{name}.<default {i}>", seen, depth + 1)
            for n, c in zip(f.__code__.co_freevars, f.__closure__ or ()):
                try:
                    self.collect(c.cell_contents, f"{name}.<{n}>", seen, depth + 1)
                except ValueError:
                    pass
            return
        for k in list(getattr(obj, "__dict__", {})) + [s for c in type(obj).__mro__ for s in getattr(c, "__slots__", ())]:
            try:
                v = getattr(obj, k) if not isinstance(getattr(type(obj), k, None), property) else None
            except Exception:
                continue
            self.collect(v, f"{name}.{k}", seen, depth + 1)

    def resolve(self, ptr):
        if self._sorted is None:
            self._sorted = sorted(self.by_base)
        i = bisect.bisect_right(self._sorted, ptr) - 1
        if i >= 0:
            al = self.by_base[self._sorted[i]]
            if ptr < al[1] + al[2]:
                return al
        return None

    def read(self, ptr, n):
        al = self.resolve(ptr)
        if al is None or ptr + n > al[1] + al[2]:
            raise LookupError(f"device table at {ptr:#x} (+{n}) lies in no known allocation")
        return bytes(byte_view(al[3])[ptr - al[1]:ptr - al[1] + n].cpu().numpy().tobytes())


def byte_view(t):
    """the whole storage of a tensor as uint8"""
    import torch
    st = t.untyped_storage()
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(st, 0, (st.nbytes(),))


# ------------------------------------------------------------------------------------------------ recorder
class _Logged:
    """the stable stand-in of one entry point (netplan._classify_bwd compares functions with `is`)"""

    def __init__(self, rec, name, real):
        self.rec, self.name, self.real = rec, name, real
        self.__name__ = getattr(real, "__name__", "mdcv_" + name)

    def __call__(self, *args):
        rc = self.real(*args)
        if self.rec.on:
            self.rec.log_call(self.name, args, rc)
        return rc


class Recorder:
    """stand-in for `mdcv._lib.lib()`: install it as `mdcv._lib._lib` before the model and its plans are built"""

    def __init__(self, real):
        self.real = real
        self.protos, self.check, self.cdll = real.protos, real.check, getattr(real, "cdll", None)
        self.directions = parse_directions()
        self.on = False
        self.trace = []
        self.step = 0
        self.entry = None                  # (list name, position, entry name) of the launch-list closure being run
        self.entry_calls = 0
        self.unmodelled = []
        self._fns = {}
        self._depth = 0
        self._keep = []                    # torch events seen: kept alive so that their id() stays theirs
        self._positions = {}

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        fn = self._fns.get(name)
        if fn is None:
            real = getattr(self.real, name)
            spec = self.directions.get(name)
            logged = spec is not None and (name in SYNC_ENTRIES or any(a[0] == "stream" for a in spec))
            fn = self._fns[name] = _Logged(self, name, real) if logged else real       # size queries and the rest pass through
        return fn

    # ---- what the stand-ins report
    @staticmethod
    def _h(s):
        s = getattr(s, "value", s)
        return int(s) if s else 0

    def log_call(self, name, args, rc):
        if name == "stream_fork":
            self.trace.append(dict(op="fork", src=self._h(args[0]), dst=self._h(args[1]), step=self.step))
        elif name == "stream_fork_arm":
            self.trace.append(dict(op="arm", src=self._h(args[0]), ev=("ring", self._h(args[2]._obj)), step=self.step))
        elif name == "stream_fork_wait":
            self.trace.append(dict(op="fwait", dst=self._h(args[0]), ev=("ring", self._h(args[1])), step=self.step))
        else:
            entry = self.entry
            if entry is None:
                entry = self._position(name, args[:-1])
            else:
                self.entry_calls += 1
            self.trace.append(dict(op="launch", name=name, args=args[:-1], stream=self._h(args[-1]), entry=entry, step=self.step, rc=rc))

    def torch_access(self, label, accesses, entry=None):
        """work torch itself enqueues on its current stream: [(label, mode, tensor)]"""
        import torch
        if not self.on:
            return
        acc = [(lab, t.data_ptr(), 1, t.numel() * t.element_size(), t.numel() * t.element_size(), mode) for lab, mode, t in accesses if t.numel()]
        self._keep += [t for _, _, t in accesses]
        self.trace.append(dict(op="launch", name=label, args=(), stream=torch.cuda.current_stream().cuda_stream, entry=entry, step=self.step,
                               acc=acc, torch=True))

    # ---- launch lists
    def _position(self, name, args):
        for lst, table in self._positions.items():
            q = table.get((name, args))
            if q:
                return (lst, q.pop(0) if len(q) > 1 else q[0], name)
        return None

    def wrap_lists(self, plan):
        """closures of the launch lists announce themselves (library entries are found by their arguments): a closure that neither makes a
        library call nor has a row in TORCH_ENTRIES is reported by name"""
        for lname in ("pre", "fwd", "bwd"):
            lst = getattr(plan, lname)
            table = self._positions[lname] = {}
            for i, (fn, args) in enumerate(lst):
                if isinstance(fn, _Logged):
                    table.setdefault((fn.name, tuple(args)), []).append(i)
                    continue
                inner = getattr(fn, "__wrapped_entry__", fn)
                lst[i] = (self._announce(inner, lname, i), args)

    def _announce(self, fn, lname, i):
        rec = self
        name = getattr(fn, "__name__", repr(fn))

        def entry(*args):
            if not rec.on:
                return fn(*args)
            rec.entry, rec.entry_calls = (lname, i, name), 0
            try:
                rc = fn(*args)
            finally:
                calls, rec.entry = rec.entry_calls, None
            if calls == 0:
                row = TORCH_ENTRIES.get(name)
                if row is None:
                    rec.unmodelled.append((lname, i, name))
                else:
                    acc = row(fn, args[:-1])
                    if acc:
                        rec.torch_access(name, acc, entry=(lname, i, name))
            return rc
        entry.__name__ = name
        entry.__wrapped_entry__ = fn
        for k in ("info", "low_water"):
            if hasattr(fn, k):
                setattr(entry, k, getattr(fn, k))
        return entry

    def unwrap(self, plan):
        """takes the announce wrappers and the run_forward / run_backward hooks off again: a plan leaves a recording as it entered it"""
        for lname in ("pre", "fwd", "bwd"):
            lst = getattr(plan, lname)
            for i, (fn, args) in enumerate(lst):
                if hasattr(fn, "__wrapped_entry__"):
                    lst[i] = (fn.__wrapped_entry__, args)
        if plan.__dict__.pop("_sched_hooked", False):
            del plan.run_forward, plan.run_backward
        self._positions = {}

    def hook_plan(self, plan):
        """enters DRIVER_OPS around the plan's run_forward / run_backward"""
        if getattr(plan, "_sched_hooked", False):
            return
        plan._sched_hooked = True
        rec, rf, rb = self, plan.run_forward, plan.run_backward
        k_in, k_out, k_grad = DRIVER_OPS

        def run_forward(x, targets=None):
            if targets is not None:
                rec.torch_access(k_in, DRIVER_OPS[k_in](plan))
            out = rf(x, targets)
            rec.torch_access(k_out, DRIVER_OPS[k_out](plan))
            return out

        def run_backward(gout):
            rec.torch_access(k_grad, DRIVER_OPS[k_grad](plan))
            return rb(gout)
        plan.run_forward, plan.run_backward = run_forward, run_backward

    # ---- torch's own synchronisation
    def patch_torch(self, mp):
        import torch
        rec = self
        S, Ev = torch.cuda.Stream, torch.cuda.Event
        o_ws, o_we, o_re, o_er = S.wait_stream, S.wait_event, S.record_event, Ev.record

        def outer(log):
            def deco(orig):
                def method(self, *a, **k):
                    rec._depth += 1
                    try:
                        out = orig(self, *a, **k)
                    finally:
                        rec._depth -= 1
                    if rec.on and rec._depth == 0:         # (wait_stream is wait_event(record_event()) in Python: the outermost call is the record)
                        log(self, out, *a, **k)
                    return out
                return method
            return deco

        def ev_id(e):
            rec._keep.append(e)
            return ("torch", id(e))
        mp.setattr(S, "wait_stream", outer(lambda s, out, other: rec.trace.append(dict(op="fork", src=other.cuda_stream, dst=s.cuda_stream, step=rec.step,
                                                                                        via="wait_stream")))(o_ws))
        mp.setattr(S, "wait_event", outer(lambda s, out, e: rec.trace.append(dict(op="wait", stream=s.cuda_stream, ev=ev_id(e), step=rec.step)))(o_we))
        mp.setattr(S, "record_event", outer(lambda s, out, event=None: rec.trace.append(dict(op="record", stream=s.cuda_stream, ev=ev_id(out),
                                                                                             step=rec.step)))(o_re))
        mp.setattr(Ev, "record", outer(lambda e, out, stream=None: rec.trace.append(dict(
            op="record", stream=(stream if stream is not None else torch.cuda.current_stream()).cuda_stream, ev=ev_id(e), step=rec.step)))(o_er))

    def resolve(self, allocs):
        """fills `acc` of every recorded library call from TABLE; -> [problem strings] (entries without a row)"""
        q = Queries(self.real, allocs.read)
        bad = []
        for r in self.trace:
            if r["op"] == "launch" and "acc" not in r:
                if r["name"] not in TABLE:
                    bad.append(f"{r['name']}: recorded in a step but has no extent row")
                    r["acc"] = []
                    continue
                r["acc"] = accesses_of(self.directions, r["name"], r["args"] + (None,), q)
        return bad


# ------------------------------------------------------------------------------------------------ analysis
class Finding:
    def __init__(self, kind, earlier=None, later=None, buffer=None, lo=0, hi=0, label="", text=""):
        self.kind, self.earlier, self.later, self.buffer, self.lo, self.hi, self.label, self.text = kind, earlier, later, buffer, lo, hi, label, text

    def __repr__(self):
        if self.kind != "hazard":
            return f"<{self.kind}: {self.text}>"
        d = lambda r: f"{r['name']}@{r.get('entry')} step {r.get('step')} trace[{r['i']}] stream {r['stream']:#x}"   # noqa: E731
        return f"<hazard {self.label}: {d(self.earlier)} -> {d(self.later)}: {self.buffer} bytes [{self.lo:#x}, {self.hi:#x})>"


class Result:
    def __init__(self):
        self.findings, self.violations = [], []
        self.launches, self.per_stream, self.forks, self.arms, self.cross_pairs = 0, {}, 0, 0, 0

    @property
    def streams(self):
        return len(self.per_stream)

    def counts(self):
        return dict(launches=self.launches, streams=self.streams, forks=self.forks, arms=self.arms, ordered_cross_stream_pairs=self.cross_pairs,
                    per_stream=dict(self.per_stream))


def analyse(trace, allocs=None):
    """trace: [record] in enqueue order -- dict(op="launch", name, stream, acc=[(label, ptr, rows, pitch, used, mode)]), dict(op="fork", src, dst),
    dict(op="arm", src, ev), dict(op="fwait", dst, ev), dict(op="record", stream, ev), dict(op="wait", stream, ev).
    allocs: Allocations, a list of (name, base, size), or None (then every pointer is its own world and sets are compared by address alone)."""
    if isinstance(allocs, (list, tuple)):
        al = Allocations()
        for n, b, s in allocs:
            al.add(n, b, s)
        allocs = al
    res = Result()
    clock = {}                             # stream -> {stream: count}
    snaps = {}                             # event -> clock snapshot
    armed = None                           # (src, event) waiting for the next library call
    launches = []

    def clk(s):
        return clock.setdefault(s, {})

    def merge(dst, src):
        d = clk(dst)
        for k, v in src.items():
            if d.get(k, 0) < v:
                d[k] = v

    for i, r in enumerate(trace):
        op = r["op"]
        if op == "launch":
            s = r["stream"]
            c = clk(s)
            c[s] = c.get(s, 0) + 1
            r["i"], r["clock"] = i, dict(c)
            res.per_stream[s] = res.per_stream.get(s, 0) + 1
            res.launches += 1
            launches.append(r)
            if armed is not None and not r.get("torch"):
                src, ev = armed
                armed = None
                if s != src:
                    res.violations.append(Finding("arm-wrong-stream", later=r, text=f"armed on {src:#x}, but the next call {r['name']} went to {s:#x}"))
                    snaps[ev] = dict(clk(src))             # (the event then rides on a foreign dispatch: nothing of `src` is behind it)
                    snaps[ev].pop(src, None)
                else:
                    snaps[ev] = dict(c)
        elif op == "fork":
            res.forks += 1
            merge(r["dst"], clk(r["src"]))
        elif op == "arm":
            res.arms += 1
            armed = (r["src"], r["ev"])
            snaps.pop(r["ev"], None)
        elif op == "fwait":
            if armed is not None and armed[1] == r["ev"]:
                res.violations.append(Finding("wait-before-call", text=f"trace[{i}]: stream_fork_wait before the armed call was made"))
                armed = None
            elif r["ev"] not in snaps:
                res.violations.append(Finding("wait-unrecorded", text=f"trace[{i}]: stream_fork_wait on an event that was never armed"))
            else:
                merge(r["dst"], snaps[r["ev"]])
        elif op == "record":
            snaps[r["ev"]] = dict(clk(r["stream"]))
        elif op == "wait":
            if r["ev"] not in snaps:
                res.violations.append(Finding("wait-unrecorded", text=f"trace[{i}]: wait_event on an event that was never recorded"))
            else:
                merge(r["stream"], snaps[r["ev"]])
        else:
            raise ValueError(f"unknown trace record {op!r}")

    # accesses by allocation
    groups = {}
    for r in launches:
        for lab, p, nrows, pitch, used, mode in r.get("acc", ()):
            al = allocs.resolve(p) if allocs is not None else ("?", 0, 1 << 62, None)
            s = (p, nrows, pitch, used)
            if al is None or hull(s)[1] > al[1] + al[2]:
                res.findings.append(Finding("unresolved", later=r, text=f"{r['name']}@{r.get('entry')}.{lab}: [{p:#x}, {hull(s)[1]:#x}) lies in no known "
                                            "allocation" + ("" if al is None else f" (runs past the end of {al[0]})")))
                continue
            groups.setdefault(al[1], (al, []))[1].append((r, lab, s, mode))
    for al, accs in groups.values():
        for j, (rb, labb, sb, mb) in enumerate(accs):
            sj = rb["stream"]
            for ra, laba, sa, ma in accs[:j]:
                if ra["stream"] == sj or ra is rb or (ma == "r" and mb == "r"):
                    continue
                ov = overlap(sa, sb, al[1])
                if ov is None:
                    continue
                res.cross_pairs += 1
                if rb["clock"].get(ra["stream"], 0) >= ra["clock"][ra["stream"]]:
                    continue
                kind = "RAW" if "w" in ma and mb == "r" else ("WAR" if ma == "r" else "WAW")
                res.findings.append(Finding("hazard", ra, rb, al[0], ov[0] - al[1], ov[1] - al[1], f"{kind} {laba} -> {labb}"))
    res.findings.sort(key=lambda f: (f.later["i"] if f.later else -1, f.earlier["i"] if f.earlier else -1))
    return res
