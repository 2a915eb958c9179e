"""-m gpu: csrc/train_log.hip (mdcv_train_log_step) through the C ABI against a NumPy / Python restatement, `==` on every word: the row's
bits, the fp64 sums as Python's own left-to-right float additions (compared with float.hex), every refusal without a launch, and guard
bands around the row and the accumulator.  Then mdcv.trainlog.StepLog on top of it: rows in step order through a ring that wraps."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mdcv import _lib, trainlog  # noqa: E402

ROW = 12
SENT = 0x5A5A5A5A
NAN = float("nan")


class Guarded:
    """`words` 32-bit words between two sentinel-filled guard bands of 64 words (the data keeps the allocation's 16-byte alignment)"""

    def __init__(self, words, guard=64):
        self.n, self.g = words, guard
        self.raw = torch.full((words + 2 * guard,), SENT, dtype=torch.int32, device="cuda")
        self.ptr = self.raw.data_ptr() + 4 * guard

    def data(self):
        return self.raw[self.g:self.g + self.n]

    def guards_intact(self):
        return bool((self.raw[:self.g] == SENT).all()) and bool((self.raw[self.g + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.raw == SENT).all())


class Acc(Guarded):
    """the fp64 accumulator [n + 1] as the caller starts it: zeros and 1e-12 in the count word"""

    def __init__(self, n):
        super().__init__(2 * (n + 1))
        self.data().view(torch.float64).copy_(torch.tensor([0.0] * n + [1e-12], dtype=torch.float64))

    def values(self):
        return self.data().view(torch.float64).cpu().tolist()


def call(losses, n, targets, with_targets, B, T, acc_ptr, row_ptr, losses_null=False):
    """one mdcv_train_log_step on the current stream; losses: device tensors or None -> the return code"""
    L = _lib.lib()
    ptrs = (ctypes.c_void_p * 8)()
    for j, t in enumerate(losses):
        ptrs[j] = None if t is None else t.data_ptr()
    tp = None if targets is None else targets.data_ptr()
    return L.train_log_step(None if losses_null else ctypes.addressof(ptrs), n, tp, with_targets, B, T, acc_ptr, row_ptr,
                            torch.cuda.current_stream().cuda_stream)


def count_targets(tg):
    """train.py:63 in plain Python: targets with more than one of their four box coordinates > 0 (a NaN is not)"""
    count = 0
    for b in range(tg.shape[0]):
        for t in range(tg.shape[1]):
            if sum(1 for v in tg[b, t, 1:5] if v > 0) > 1:
                count += 1
    return count


def expected(loss_values, tg, acc):
    """-> (row as float32 [ROW], the accumulator after the step): Python floats, the loop's own additions in its order"""
    n = len(loss_values)
    count = 0 if tg is None else count_targets(tg)
    row = np.zeros(ROW, np.float32)
    acc = list(acc)
    for j, v in enumerate(loss_values):
        v32 = np.float32(0.0 if v is None else v)
        row[j] = v32
        acc[j] += float(v32)
    row[n] = np.float32(count)
    step_num_targets = count + 1e-12
    acc[n] += step_num_targets
    return row, acc


def dev_losses(values):
    return [None if v is None else torch.tensor(v, dtype=torch.float32, device="cuda") for v in values]


def check_step(loss_values, tg, with_targets=1, acc=None, shape=None):
    """one launch against the restatement, every word; -> the Acc for a next launch"""
    n = len(loss_values)
    acc = acc or Acc(n)
    before = acc.values()
    row = Guarded(ROW)
    B, T = shape if shape is not None else ((0, 0) if tg is None else tg.shape[:2])
    tdev = None if tg is None or tg.size == 0 else torch.from_numpy(tg).cuda()
    src = dev_losses(loss_values)
    assert call(src, n, tdev, with_targets, B, T, acc.ptr, row.ptr) == 0
    torch.cuda.synchronize()
    want_row, want_acc = expected(loss_values, tg if with_targets else None, before)
    got_row = row.data().cpu().numpy()
    assert (got_row == want_row.view(np.int32)).all(), (got_row.view(np.float32), want_row)
    assert [float.hex(v) for v in acc.values()] == [float.hex(v) for v in want_acc]
    assert row.guards_intact() and acc.guards_intact()
    return acc


CRAFTED = np.array([
    # class, x, y, w, h                                                         positive coordinates
    [[0, 0.5, 0.5, 0.1, 0.2], [0, 0.0, 0.0, 0.0, 0.0], [3, 0.0, 0.0, 0.0, 0.0], [1, 0.7, 0.0, 0.0, 0.0], [0, 0.0, 0.0, 0.0, 0.0]],      # 4 0 0 1 0
    [[0, 0.2, 0.0, 0.3, 0.0], [0, -0.5, -0.5, 0.1, -0.2], [0, -1.0, 0.4, 0.6, -0.0], [0, 0.0, 0.0, 0.0, 0.0], [0, 0.0, 0.0, 0.0, 0.0]],  # 2 1 2 0 0
    [[0, NAN, NAN, 0.5, 0.5], [0, NAN, NAN, NAN, 0.5], [0, NAN, NAN, NAN, NAN], [5, 1e-45, 0.0, 0.0, 3e38], [9, 0.0, 0.0, 0.0, 1.0]],    # 2 1 0 2 1
], np.float32)
SEVEN = [13.708738, 0.5524507, 0.6181793, 0.12075743, 0.0986148, 11.921195, 0.39754093]


def test_one_target():
    assert count_targets(np.array([[[0, 0.5, 0.5, 0, 0]]], np.float32)) == 1
    check_step(SEVEN, np.array([[[0, 0.5, 0.5, 0.0, 0.0]]], np.float32))
    check_step(SEVEN, np.array([[[2, 0.5, 0.0, 0.0, 0.0]]], np.float32))


def test_crafted_targets_zero_one_two_four_positive_negative_and_nan():
    assert count_targets(CRAFTED) == 5                     # rows with 4, 2, 2, 2, 2 positive coordinates
    check_step(SEVEN, CRAFTED)
    check_step([1.5], CRAFTED)                             # one loss: the count sits in word 1
    check_step([0.1 * k for k in range(8)], CRAFTED)       # eight: the count sits in word 8


@pytest.mark.parametrize("shape", [(0, 5), (4, 0), (0, 0)])
def test_no_targets_in_the_batch(shape):
    check_step(SEVEN, np.zeros(shape + (5,), np.float32), shape=shape)


def test_targets_not_requested_and_a_null_source():
    check_step([0.27184075, None, 0.27184075], None, with_targets=0)
    check_step([0.27184075, None, 0.27184075], CRAFTED, with_targets=0)      # a pointer that was not asked for is not read: count 0


def test_more_than_one_pass_of_the_workgroup():
    g = np.random.default_rng(7)
    tg = g.random((8, 300, 5), dtype=np.float32)
    tg[:, :, 1:] -= 0.55                                   # about 60 % of the rows have more than one positive coordinate
    tg[:, 200:] = 0                                        # zero padding rows, as the loaders pad
    tg[3, 17, 2] = NAN
    c = count_targets(tg)
    assert 300 < c < 1200
    check_step(SEVEN, tg)


def test_nan_and_infinite_losses_pass_through():
    check_step([NAN, float("inf"), -0.0, 1e-45, 3e38, -1.0, 0.0], CRAFTED)


def test_three_launches_add_up_like_python():
    g = np.random.default_rng(11)
    acc = None
    py_losses, py_targets = [0.0] * 7, 1e-12
    for k in range(3):
        vals = [float(np.float32(v)) for v in g.random(7) * [40, 1, 1, 1, 1, 30, 2]]
        tg = g.random((3, 6, 5), dtype=np.float32) - 0.4
        acc = check_step(vals, tg, acc=acc)
        for j in range(7):
            py_losses[j] += vals[j]                        # epoch_losses[j] += batch_loss
        step_num_targets = count_targets(tg) + 1e-12
        py_targets += step_num_targets                     # epoch_num_targets += step_num_targets
    got = acc.values()
    assert [float.hex(v) for v in got[:7]] == [float.hex(v) for v in py_losses]
    assert float.hex(got[7]) == float.hex(py_targets)


def test_every_refusal_comes_before_any_launch():
    acc, row = Acc(7), Guarded(ROW)
    before = acc.values()
    src = dev_losses(SEVEN)
    tg = torch.from_numpy(CRAFTED).cuda()
    bad = [
        call(src, 7, tg, 1, 3, 5, None, row.ptr),                       # acc NULL
        call(src, 7, tg, 1, 3, 5, acc.ptr, None),                       # row NULL
        call(src, 7, tg, 1, 3, 5, acc.ptr, row.ptr, losses_null=True),  # no table of sources
        call(src, 0, tg, 1, 3, 5, acc.ptr, row.ptr),
        call(src, 9, tg, 1, 3, 5, acc.ptr, row.ptr),
        call(src, -1, tg, 1, 3, 5, acc.ptr, row.ptr),
        call(src, 7, tg, 1, -1, 5, acc.ptr, row.ptr),
        call(src, 7, tg, 1, 3, -5, acc.ptr, row.ptr),
        call(src, 7, tg, 0, -3, 5, acc.ptr, row.ptr),                   # negative also when targets were not requested
        call(src, 7, None, 1, 3, 5, acc.ptr, row.ptr),                  # requested, B*T > 0, no pointer
        call(src, 7, tg, 1, 65536, 65536, acc.ptr, row.ptr),            # B*T beyond int
    ]
    torch.cuda.synchronize()
    assert bad == [-1] * len(bad)
    assert row.untouched() and acc.guards_intact() and acc.values() == before
    assert call(src, 7, None, 1, 0, 5, acc.ptr, row.ptr) == 0           # requested, but B*T == 0: no pointer needed
    torch.cuda.synchronize()
    assert row.guards_intact() and not row.untouched()


# ---------------------------------------------------------------------------------------------------------------- StepLog
@pytest.mark.parametrize("ring", [2, 64])
def test_steplog_rows_in_order_and_sums(ring):
    got = []
    log = trainlog.StepLog(3, ring=ring, on_row=lambda i, row, meta: got.append((i, row, meta)))
    g = np.random.default_rng(3)
    want_rows, sums = [], [0.0, 0.0, 0.0, 1e-12]
    for i in range(7):
        vals = [float(np.float32(v)) for v in g.random(3)]
        tg = g.random((2, 4, 5), dtype=np.float32) - 0.3
        log.drain()
        src = dev_losses(vals)
        log.record([src[0], None, src[2]], torch.from_numpy(tg).cuda(), meta="step %d" % i)
        c = count_targets(tg)
        want_rows.append((i, [vals[0], 0.0, vals[2], float(c)], "step %d" % i))
        sums[0] += vals[0]
        sums[2] += vals[2]
        sums[3] += c + 1e-12
    log.drain(block=True)
    assert got == want_rows
    assert [float.hex(v) for v in log.sums()] == [float.hex(v) for v in sums]
    if ring == 64:
        assert log.host_waits == 1
    log.reset()                                            # the next epoch starts from 0.0 / 1e-12 and step 0
    log.record(dev_losses([1.0, 2.0, 3.0]), None)
    assert log.sums() == [1.0, 2.0, 3.0, 1e-12 + (0 + 1e-12)] and got[-1][0] == 0


def test_steplog_refuses_host_tensors_and_wrong_counts():
    log = trainlog.StepLog(3)
    with pytest.raises(ValueError):
        log.record([torch.tensor(0.0)] * 3)
    with pytest.raises(ValueError):
        log.record(dev_losses([1.0, 2.0]))
    with pytest.raises(ValueError):
        log.record(dev_losses([1.0, 2.0, 3.0]), torch.zeros(2, 4, 4, device="cuda"))
    with pytest.raises(ValueError):
        trainlog.StepLog(9)
