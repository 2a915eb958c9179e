"""One batch: its byte layout in the staging buffer, the pack, and the launches (csrc/imgload.hip's pair, csrc/imgaug.hip's three or
four for a batch with an augmented sample, one more of csrc/imgfx.hip for a batch with a blurred / noised / contrasted / sharpened one)."""
import numpy as np
import torch

from ... import _lib
from ..staging import Layout as _Layout, align as _align
from .augment import AUG_DESC, FX_DESC, aug_descriptor, fx_descriptor, sigmoid_table
from .geometry import crop_window, frame_reference

DESC = 20                                # MDCV_IMGLOAD_DESC
FREF = 4                                 # MDCV_IMGLOAD_FREF
STAGED = (-1, 0, 0, 0)                   # a frame reference that says: this image's window is in the staging buffer


class Layout(_Layout):
    """Sections present only when a sample needs them: `aug` / `fref` / `fx` say whether [augmentation descriptors] / [frame
    references] / [fx descriptors][contrast tables] are laid out (their offsets exist only then); `n_luts` counts the tables."""
    aug = fref = fx = False
    n_luts = 0


def pack_layout(geoms, windows_nbytes, num_targets, frefs=None):
    """Byte layout of one batch's staging buffer: [descriptors][labels][coefficient tables][pixels], and behind them, only when a
    sample of the batch is augmented, [augmentation descriptors] (a batch without one is laid out exactly as before).  `frefs` (one
    frame reference per sample, `STAGED` for a staged one; a pooled sample's window has 0 bytes): the batch reads a frame cache, and
    [frame references] follow.  Only when a sample has an imgaug op, [fx descriptors][contrast tables] come last."""
    p = Layout()
    B = len(geoms)
    p.B, p.T = B, num_targets
    p.desc_off, p.lab_off = 0, _align(B * DESC * 4)
    p.coef_off = _align(p.lab_off + B * num_targets * 5 * 4)
    n_coef = sum(g.col.size + g.row.size for g in geoms)
    p.n_coefs = max(n_coef, 1)
    p.pix_off = _align(p.coef_off + p.n_coefs * 4)
    p.src_bytes = sum(windows_nbytes)
    p.nbytes = _align(p.pix_off + p.src_bytes)
    p.aug = any(bool(g.aug) for g in geoms)
    if p.aug:
        p.aug_off = p.nbytes
        p.nbytes = _align(p.aug_off + B * AUG_DESC * 4)
    p.fref = frefs is not None
    if p.fref:
        p.fref_off = p.nbytes
        p.nbytes = _align(p.fref_off + B * FREF * 8)
    p.fx = any(bool(g.fx) and g.fx.runs() for g in geoms)
    if p.fx:
        p.n_luts = sum(1 for g in geoms if g.fx and g.fx.contrast is not None)
        p.fx_off = p.nbytes
        p.lut_off = _align(p.fx_off + B * FX_DESC * 4)
        p.nbytes = _align(p.lut_off + p.n_luts * 256)
    p.max_scr_w = max(g.desc[7] for g in geoms)
    p.max_scr_h = max(g.desc[8] for g in geoms)
    return p


def pack_batch(buf, p, geoms, windows, labels=None, frefs=None):
    """Fill a uint8 numpy buffer of at least p.nbytes bytes (the pinned staging) with the batch; a pooled sample's window is None."""
    desc = buf[p.desc_off:p.desc_off + p.B * DESC * 4].view(np.int32).reshape(p.B, DESC)
    coefs = buf[p.coef_off:p.coef_off + p.n_coefs * 4].view(np.int32)
    c, s = 0, 0
    for b, (g, w) in enumerate(zip(geoms, windows)):
        d = list(g.desc)
        d[0] = s
        d[5] = c
        coefs[c:c + g.col.size] = g.col.reshape(-1)
        c += g.col.size
        d[6] = c
        coefs[c:c + g.row.size] = g.row.reshape(-1)
        c += g.row.size
        desc[b] = d
        if w is not None:
            buf[p.pix_off + s:p.pix_off + s + w.nbytes] = w.reshape(-1)
            s += w.nbytes
    if p.aug:
        aug = buf[p.aug_off:p.aug_off + p.B * AUG_DESC * 4].view(np.int32).reshape(p.B, AUG_DESC)
        for b, g in enumerate(geoms):
            aug[b] = aug_descriptor(g.aug)
    if p.fref:
        buf[p.fref_off:p.fref_off + p.B * FREF * 8].view(np.int64).reshape(p.B, FREF)[:] = np.asarray(frefs, np.int64).reshape(p.B, FREF)
    if p.fx:
        fxd = buf[p.fx_off:p.fx_off + p.B * FX_DESC * 4].view(np.int32).reshape(p.B, FX_DESC)
        luts = buf[p.lut_off:p.lut_off + p.n_luts * 256].reshape(p.n_luts, 256)
        n = 0
        for b, g in enumerate(geoms):
            fxd[b] = fx_descriptor(g.fx, n)
            if g.fx and g.fx.contrast is not None:
                luts[n] = sigmoid_table(*g.fx.contrast)
                n += 1
    if p.T and labels is not None:
        buf[p.lab_off:p.lab_off + p.B * p.T * 20].view(np.float32)[:] = np.asarray(labels, np.float32).reshape(-1)


def launch_batch(dev_buf, host_buf, p, channels, height, width, stream, pool=None):
    """Enqueue the kernels on `stream` for a staged batch already copied to `dev_buf` (device uint8) -> imgs [B,C,H,W]: the pair of
    csrc/imgload.hip, or csrc/imgaug.hip's sequence when the batch carries augmentation descriptors.  A batch with frame references
    goes through the two `_frames_` entry points with `pool` (device uint8, or None): the same launches.  A batch with fx descriptors
    gets csrc/imgfx.hip's one launch behind them, out of place into a second batch buffer allocated here."""
    imgs = _launch_load(dev_buf, host_buf, p, channels, height, width, stream, pool)
    if not p.fx:
        return imgs
    if channels != 3:
        raise ValueError("blur / noise / contrast / sharpen need RGB batches (bw=False)")
    out = torch.empty_like(imgs)
    base, hb = dev_buf.data_ptr(), host_buf.ctypes.data
    L = _lib.lib()
    L.check(L.imgfx_batch(hb + p.fx_off, base + p.fx_off, p.B, base + p.lut_off if p.n_luts else None, p.n_luts, channels, height, width,
                          imgs.data_ptr(), out.data_ptr(), stream.cuda_stream), "imgfx_batch")
    return out


def _launch_load(dev_buf, host_buf, p, channels, height, width, stream, pool):
    """mdcv_imgload[_aug][_frames]_batch: one argument list, the optional parts in the order the four entry points share"""
    L = _lib.lib()
    dev = dev_buf.device
    imgs = torch.empty(p.B, channels, height, width, dtype=torch.float32, device=dev)
    wsb = L.imgload_workspace_bytes(p.B, p.max_scr_w, p.max_scr_h)
    work = [torch.empty(max(int(wsb), 1), dtype=torch.uint8, device=dev)]
    base, hb = dev_buf.data_ptr(), host_buf.ctypes.data
    tables, source = [hb + p.desc_off, base + p.desc_off], [base + p.pix_off, p.src_bytes]
    if p.fref:
        tables += [hb + p.fref_off, base + p.fref_off]
        source += [pool.data_ptr() if pool is not None else None, int(pool.numel()) if pool is not None else 0]
    if p.aug:
        awb = L.imgaug_workspace_bytes(p.B, height, width)
        if awb < 0:
            raise ValueError(f"augmented batches need 0 < H * W <= 4096 * 4096, got {height}x{width}")
        tables += [hb + p.aug_off, base + p.aug_off]
        work.append(torch.empty(int(awb), dtype=torch.uint8, device=dev))
    name = "imgload" + ("_aug" if p.aug else "") + ("_frames" if p.fref else "") + "_batch"
    L.check(getattr(L, name)(*tables, p.B, base + p.coef_off, p.n_coefs, *source, p.max_scr_w, p.max_scr_h, channels, height, width,
                             *(w.data_ptr() for w in work), imgs.data_ptr(), stream.cuda_stream), name)
    return imgs


def transform_batch(frames, geoms, bw=False, device=None, pool=None, offsets=None):
    """Synchronous convenience (tests, probes): decoded frames [(H, W, 3) uint8] + their geometries (each may carry `.aug`, an
    `Augmentation` with its matrix set, and `.fx`, an `ImageFx`) -> imgs [B,C,H,W] fp32 on the device.  With `pool` (device uint8) and
    `offsets` (per sample: the byte offset in `pool` at which its whole frame already lies, rows of 3 * frame width bytes; None: stage
    the window from `frames`), pooled samples are read in place and their entry of `frames` is not looked at."""
    _lib.require_gpu()
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    offsets = [None] * len(geoms) if pool is None else offsets
    frefs = None if pool is None else [STAGED if o is None else frame_reference(g, o) for g, o in zip(geoms, offsets)]
    windows = [crop_window(f, g) if o is None else None for f, g, o in zip(frames, geoms, offsets)]
    p = pack_layout(geoms, [0 if w is None else w.nbytes for w in windows], 0, frefs)
    host = np.zeros(p.nbytes, np.uint8)
    pack_batch(host, p, geoms, windows, frefs=frefs)
    with torch.cuda.device(device):
        dev = torch.from_numpy(host).to(device)
        return launch_batch(dev, host, p, 1 if bw else 3, geoms[0].height, geoms[0].width, torch.cuda.current_stream(device), pool)
