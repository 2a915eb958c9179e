"""Frame cache, host half (no GPU): static admission, the decode-once rule under threads, the staging layout of a batch that reads the pool,
and the frame-reference validator of the two `_frames_` entry points, which runs on the host copies before anything is enqueued."""
import os
import sys
import threading
import time
import warnings
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from mdcv.data import framecache as F
from mdcv.data import images as I

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import imgaug_cases as K  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imgload")
# dataset.csv: f0 301x173 (6 patches at 64x64), f1 97x211 (2), f2 257x129 (1), f3 120x90 (2)
NBYTES = {"f0.png": 3 * 301 * 173, "f1.png": 3 * 97 * 211, "f2.png": 3 * 257 * 129, "f3.png": 3 * 120 * 90}


def _loader(**kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return I.ImageLabelBatches(os.path.join(G, "dataset.csv"), "", 64, 64, ts=True, batch_size=4, **kw)


def _r(n):
    return (n + 255) // 256 * 256


def test_admission_is_aligned_disjoint_in_csv_order_and_keyed_by_path():
    ld = _loader(cache_bytes=1 << 30)
    assert len(ld.img_files) == 11                                    # one entry per patch ...
    ents = ld._cache.entries
    assert list(ents) == ["f0.png", "f1.png", "f2.png", "f3.png"]     # ... one slot per path, in CSV order
    top = 0
    for name, e in ents.items():
        assert e.offset == top and e.offset % 256 == 0 and e.nbytes == NBYTES[name]
        top += _r(e.nbytes)
    st = ld.cache_stats()
    assert st["bytes_reserved"] == top == sum(_r(n) for n in NBYTES.values()) and st["pool_bytes"] == 0     # no allocation before iteration
    assert st["hits"] == st["fills"] == 0 and st["misses"] == dict(not_admitted=0, size_mismatch=0)
    assert _loader().cache_stats() is None and _loader()._cache is None


def test_a_file_that_does_not_fit_is_skipped_and_a_later_small_one_admitted():
    budget = _r(NBYTES["f0.png"]) + _r(NBYTES["f3.png"])
    ents = _loader(cache_bytes=budget)._cache.entries
    assert list(ents) == ["f0.png", "f3.png"] and ents["f3.png"].offset == _r(NBYTES["f0.png"])
    assert _loader(cache_bytes=budget - 1)._cache.entries.keys() == {"f0.png"}          # rounded sizes count, to the byte
    ld = _loader(cache_bytes=0)
    assert ld._cache.entries == {} and ld.cache_stats()["bytes_reserved"] == 0
    with pytest.raises(ValueError):
        _loader(cache_bytes=-1)


def test_admission_does_not_depend_on_shuffle_or_seed():
    budget = _r(NBYTES["f0.png"]) + _r(NBYTES["f2.png"]) + 100
    want = None
    for shuffle in (False, True):
        for seed in (0, 1, 12345):
            ld = _loader(cache_bytes=budget, shuffle=shuffle, seed=seed)
            got = {k: (e.offset, e.nbytes, e.size) for k, e in ld._cache.entries.items()}
            want = want or got
            assert got == want and list(got) == ["f0.png", "f1.png", "f3.png"]       # f1 takes room f2 then lacks; f3 still fits


def test_limit_caps_the_last_slot_end():
    slots, top = F.admit(["a", "b", "c"], [(10, 10), (100, 100), (10, 10)], 1 << 40, limit=1024)
    assert list(slots) == ["a", "c"] and top == 1024 and slots["c"][0] == 512            # reservations are whole 256-byte units
    assert list(F.admit(["a", "b", "c"], [(10, 10), (100, 100), (10, 10)], 1 << 40, limit=1023)[0]) == ["a"]


def test_each_admitted_file_is_decoded_once_under_threads():
    calls, gate = Counter(), threading.Barrier(8)
    sizes = {"a": (31, 7), "b": (5, 9), "c": (4, 4)}

    def decode(path):
        calls[path] += 1
        time.sleep(0.01)                                              # long enough for every other thread to arrive at the lock
        w, h = sizes[path] if path != "c" else (5, 4)                 # c decodes to another size than planned
        return np.full((h, w, 3), ord(path), np.uint8)

    cache = F.FrameCache(["a", "a", "b", "c", "d"], [sizes["a"], sizes["a"], sizes["b"], sizes["c"], (1 << 20, 1 << 20)], 4096)
    assert list(cache.entries) == ["a", "b", "c"]                     # d does not fit

    def ask(path):
        gate.wait()
        return cache.lookup(path, decode)

    with ThreadPoolExecutor(8) as pool:
        got = list(pool.map(ask, ["a"] * 5 + ["b"] * 3))
    assert calls == {"a": 1, "b": 1}
    assert all(e is cache.entries[p] and f is None for (e, f), p in zip(got, ["a"] * 5 + ["b"] * 3))
    st = cache.stats()
    assert st["fills"] == 2 and st["hits"] == 6
    fills = cache.take_fills([e for e, _ in got])
    assert sorted(e.path for e in fills) == ["a", "b"] and cache.take_fills([e for e, _ in got]) == []      # each goes up once
    assert fills[0].frame.shape == (7, 31, 3) and fills[0].frame.flags.c_contiguous
    cache.restart()                                                   # an abandoned epoch: staged frames go up with their next batch
    assert len(cache.take_fills([e for e, _ in got])) == 2
    cache.filled(fills, "event")
    assert all(e.frame is None and e.state == F.FILLED for e in fills) and cache.last_fill == "event"
    # a size mismatch is never cached and decoded every time; a file that was not admitted likewise
    for k in range(3):
        e, f = cache.lookup("c", decode)
        assert e is None and f.shape == (4, 5, 3)
        e, f = cache.lookup("d", lambda p: np.zeros((2, 2, 3), np.uint8))
        assert e is None and f.shape == (2, 2, 3)
    assert calls["c"] == 3
    assert cache.stats()["misses"] == dict(not_admitted=3, size_mismatch=3)


def test_a_pooled_sample_stages_no_pixels_and_its_reference_names_the_window():
    ld = _loader(cache_bytes=1 << 30, lr_flip=True, data_aug=True)
    z = np.load(os.path.join(G, "frames.npz"))
    ld.decode = lambda p: z[os.path.splitext(os.path.basename(p))[0]]
    got = [ld._sample(0, i) for i in (0, 6, 8)]                       # f0, f1, f2
    assert all(w is None and e is not None for _, w, e in got)
    geoms = [g for g, _, _ in got]
    frefs = [I.frame_reference(g, e.offset) for g, _, e in got]
    for g, e, f in zip(geoms, [e for _, _, e in got], frefs):
        x, y, w, h = g.window
        assert f == (e.offset, 3 * g.frame[0], x, y) and x >= 0 and y >= 0 and w > 0 and h > 0
        assert f[0] + (y + h - 1) * f[1] + 3 * (x + w) <= e.offset + e.nbytes
    plain = I.pack_layout(geoms, [0, 0, 0], ld.num_targets_per_image)
    p = I.pack_layout(geoms, [0, 0, 0], ld.num_targets_per_image, frefs)
    assert p.src_bytes == 0 and p.fref and p.fref_off == plain.nbytes and p.nbytes == plain.nbytes + I._align(3 * I.FREF * 8)
    buf = np.zeros(p.nbytes, np.uint8)
    I.pack_batch(buf, p, geoms, [None] * 3, [g.labels for g in geoms], frefs)
    assert np.array_equal(buf[p.fref_off:p.fref_off + 96].view(np.int64).reshape(3, 4), np.array(frefs, np.int64))
    assert (buf[:3 * I.DESC * 4].view(np.int32).reshape(3, I.DESC)[:, 0] == 0).all()
    # the same samples without a cache: same plan, and the window bytes are what the reference names
    ref = _loader(lr_flip=True, data_aug=True)
    ref.decode = ld.decode
    for (g, _, e), i in zip(got, (0, 6, 8)):
        g0, w0, _ = ref._sample(0, i)
        assert g0.desc == g.desc and np.array_equal(g0.labels, g.labels)
        x, y, w, h = g.window
        assert np.array_equal(w0, e.frame[y:y + h, x:x + w])
    # an empty window (pad-and-resize never has one here; built by hand): origin (0, 0) whatever the geometry says
    g = geoms[0]
    g.window = (-5, 3, 0, 7)
    assert I.frame_reference(g, 512) == (512, 3 * g.frame[0], 0, 0)


def test_the_entry_points_validate_frame_references_on_the_host_copies():
    """Bad references come back as MDCV_EARG from the host tables alone, as in tests/test_kptload_host.py; a good one passes the validator.
    A call that passes goes on to its launches: with a GPU in the machine the buffers are real device copies and it returns 0, without one
    the launch fails with HIP's own error code, which is not MDCV_EARG."""
    import torch
    from mdcv import _lib
    L = _lib.lib()
    gpu = torch.cuda.is_available()
    frs = K.frames()
    c = [c for c in K.cases()[0] if c["ts"] and c["jitter"] and c["affine"] and (c["W"], c["H"]) == (64, 64) and c["u8"].shape[2] == 3
         and c["name"] == "f0"][0]
    g = K.geometry(I, c, frs)
    x0, y0, w, h = g.window
    assert (x0 > 0 or y0 > 0) and w > 0 and h > 0
    f = frs["f0"]
    off, pitch = 13, 3 * f.shape[1]                                   # an odd offset, a pitch that is no multiple of 4
    assert pitch % 4 != 0
    pool = np.concatenate([np.full(off, 0xEE, np.uint8), f.reshape(-1)])
    end = off + (y0 + h - 1) * pitch + 3 * (x0 + w)                   # one past the window's last byte
    good = (off, pitch, x0, y0)
    keep = []

    def device(a):
        """what stands for the device copy of `a`: a real one when there is a GPU"""
        if not gpu:
            return a.ctypes.data
        keep.append(torch.from_numpy(a).cuda())
        return keep[-1].data_ptr()

    def batch(window, fref):
        p = I.pack_layout([g], [0 if window is None else window.nbytes], 0, [fref])
        host = np.zeros(p.nbytes, np.uint8)
        I.pack_batch(host, p, [g], [window], frefs=[fref])
        return p, host, device(host)
    p, host, base = batch(None, good)
    ps, hosts, bases = batch(I.crop_window(f, g), I.STAGED)
    pool_dev = device(pool)
    out = device(np.zeros(3 * 64 * 64, np.float32))
    ws = device(np.zeros(max(int(L.imgload_workspace_bytes(1, p.max_scr_w, p.max_scr_h)), 1), np.uint8))
    aws = device(np.zeros(int(L.imgaug_workspace_bytes(1, 64, 64)), np.uint8))
    st = torch.cuda.current_stream().cuda_stream if gpu else None

    def run(augmented, ref=good, pool_bytes=pool.size, d=None, fref_host=True, staged=False):
        q, hb, db = (ps, hosts, bases) if staged else (p, host, base)
        r = np.array(ref, np.int64)
        d = np.ascontiguousarray(hb[:I.DESC * 4].view(np.int32) if d is None else d, np.int32)
        rh = r.ctypes.data if fref_host else None
        src = (db + q.pix_off, q.src_bytes, pool_dev, pool_bytes)
        if augmented:
            return L.imgload_aug_frames_batch(d.ctypes.data, db + q.desc_off, rh, db + q.fref_off, hb.ctypes.data + q.aug_off, db + q.aug_off,
                                              1, db + q.coef_off, q.n_coefs, *src, q.max_scr_w, q.max_scr_h, 3, 64, 64, ws, aws, out, st)
        return L.imgload_frames_batch(d.ctypes.data, db + q.desc_off, rh, db + q.fref_off, 1, db + q.coef_off, q.n_coefs, *src, q.max_scr_w,
                                      q.max_scr_h, 3, 64, 64, ws, out, st)

    bad = dict(off_minus_2=dict(ref=(-2, pitch, x0, y0)), one_byte_past_the_pool=dict(pool_bytes=end - 1),
               pitch_one_short=dict(ref=(off, 3 * (x0 + w) - 1, x0, y0)), negative_x0=dict(ref=(off, pitch, -1, y0)),
               negative_y0=dict(ref=(off, pitch, x0, -1)), wrapping_product=dict(ref=(0, 1 << 62, 0, 4)), no_host_table=dict(fref_host=False),
               staged_row_without_staged_bytes=dict(ref=I.STAGED))
    empty = host[:I.DESC * 4].view(np.int32).copy()
    empty[1:3] = 0                                                    # an empty window: nothing is read, the reference need name no byte
    passes = dict(whole_pool=dict(), to_the_byte=dict(pool_bytes=end), empty_window=dict(d=empty, ref=(end, 0, 0, 0), pool_bytes=end),
                  staged_row=dict(ref=I.STAGED, staged=True))
    for augmented in (False, True):
        for what, kw in bad.items():
            assert run(augmented, **kw) == -1, (augmented, what)
        for what, kw in passes.items():
            rc = run(augmented, **kw)
            assert rc == 0 if gpu else rc != -1, (augmented, what, rc)
    if gpu:
        torch.cuda.synchronize()
