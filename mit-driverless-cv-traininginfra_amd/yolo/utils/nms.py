"""GPU drop-in for the reference's CVC-YOLOv3/utils/nms.py (`nms`, nms.py:4-61).

Same signature and return value (the kept indices with respect to `boxes`, highest score first) but the whole greedy
loop runs in one HIP workgroup (csrc/postprocess.hip): radix-select of the top_k scores, LDS sort, a 64-bit suppression
matrix built with wave ballots and a single-wave scan over it.  No CPU fallback.
"""
import torch

from ... import _lib

MAX_TOPK = 512


def _check_classes(who, scores, classes):
    n = int(scores.shape[0])
    if classes is not None and (classes.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
                                or classes.dim() != 1 or int(classes.shape[0]) != n):
        raise ValueError(f"{who}: classes must be an integer tensor of length {n}, got {classes.dtype} {list(classes.shape)}")
    return n


def nms(boxes, scores, overlap=0.5, top_k=200, classes=None, *, method="hard", sigma=0.5, score_thres=0.0):
    """boxes [n,4] corner format, scores [n], both on the GPU.  Returns a LongTensor of kept indices.

    classes: an integer tensor [n] selects the class-aware scan (csrc/detect_mc.hip): the top_k scores are selected as
    before, and a kept box removes a later one of ITS class only; the kept indices come back in the same visiting order.

    Equal scores are visited by descending index (what the reference's ascending sort + walk-from-the-back gives with a
    stable sort; its CPU sort is not stable past 16 elements, so ties are implementation-defined there).
    Reading the number of kept boxes back costs one device sync, like the reference's dynamic-shape loop.

    method="linear" | "gaussian": `soft_nms`'s keep list, in descending decayed score; the caller's tensors stay as
    they are.  "hard" is the path above."""
    if _lib.nms_method("nms", method, sigma):
        return soft_nms(boxes, scores, overlap, top_k, method, sigma, score_thres, classes)[0]
    n = _check_classes("nms", scores, classes)
    _lib.require_gpu(scores)
    L = _lib.lib() if classes is None else _lib.mcdet_lib()
    dev = scores.device
    if boxes.numel() == 0:                                   # nms.py:17-18 returns the (empty) keep buffer
        return torch.zeros(n, dtype=torch.long, device=dev)
    if not 0 < int(top_k) <= MAX_TOPK:
        raise ValueError(f"nms: top_k must be in 1..{MAX_TOPK} (got {top_k})")
    bx = boxes.detach().to(torch.float32).contiguous()
    sc = scores.detach().to(torch.float32).contiguous()
    keep = torch.empty(min(n, int(top_k)), dtype=torch.long, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    if classes is not None:
        cl = classes.detach().to(device=dev, dtype=torch.int32).contiguous()
        ws = torch.empty(int(L.nms_mc_workspace_bytes(n)), dtype=torch.uint8, device=dev)
        L.check(L.nms_mc(bx.data_ptr(), sc.data_ptr(), cl.data_ptr(), n, float(overlap), int(top_k), keep.data_ptr(), count.data_ptr(),
                         ws.data_ptr(), torch.cuda.current_stream().cuda_stream), "nms_mc")
        return keep[:int(count.item())]
    ws = torch.empty(int(L.nms_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    L.check(L.nms(bx.data_ptr(), sc.data_ptr(), n, float(overlap), int(top_k), keep.data_ptr(), count.data_ptr(), ws.data_ptr(),
                  torch.cuda.current_stream().cuda_stream), "nms")
    return keep[:int(count.item())]


def soft_nms(boxes, scores, overlap=0.5, top_k=200, method="linear", sigma=0.5, score_thres=0.0, classes=None):
    """Soft-NMS (Bodla et al. 2017) in one HIP workgroup (csrc/soft_nms.hip; include/mdcv_softnms.h states the rule).

    boxes [n,4] corner format and scores [n] on the GPU -> (keep, decayed_scores): the indices with respect to `boxes` in the order
    they were picked, which is descending decayed score, and those scores.  method "linear" multiplies the score of a box whose IoU
    with the pick exceeds `overlap` by 1 - IoU, "gaussian" every overlapping box's by exp(-IoU^2 / sigma), "hard" removes as `nms`
    does; a soft scan ends at the first pick that is not above score_thres.  classes [n]: only boxes of the pick's class decay."""
    code = _lib.nms_method("soft_nms", method, sigma)
    if float(score_thres) != float(score_thres):
        raise ValueError("soft_nms: score_thres is NaN")
    n = _check_classes("soft_nms", scores, classes)
    _lib.require_gpu(scores)
    L = _lib.softnms_lib()
    dev = scores.device
    if not 0 < int(top_k) <= MAX_TOPK:
        raise ValueError(f"soft_nms: top_k must be in 1..{MAX_TOPK} (got {top_k})")
    if n == 0:
        return torch.zeros(0, dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.float32, device=dev)
    bx = boxes.detach().to(torch.float32).contiguous()
    sc = scores.detach().to(torch.float32).contiguous()
    cl = None if classes is None else classes.detach().to(device=dev, dtype=torch.int32).contiguous()
    keep = torch.empty(min(n, int(top_k)), dtype=torch.long, device=dev)
    out = torch.empty(min(n, int(top_k)), dtype=torch.float32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.soft_nms_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    L.check(L.soft_nms(bx.data_ptr(), sc.data_ptr(), None if cl is None else cl.data_ptr(), n, code, float(overlap), float(sigma),
                       float(score_thres), int(top_k), keep.data_ptr(), out.data_ptr(), count.data_ptr(), ws.data_ptr(),
                       torch.cuda.current_stream().cuda_stream), "soft_nms")
    c = int(count.item())
    return keep[:c], out[:c]
