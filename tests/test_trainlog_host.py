"""Host half of the native training loops (no GPU): the formatters of mdcv.yolo.train / mdcv.rektnet.train against the reference's
statements, restated here on recorded rows, and the slot / order logic of mdcv.trainlog.RowRing under a fake event that lands late."""
import pytest

from mdcv.trainlog import RowRing
from mdcv.yolo.train import format_step_line
from mdcv.rektnet.train import format_batch_description, format_epoch_line


class _Item:
    """stands in for a 0-dim loss tensor of the reference's loop: `.item()` gives the recorded number"""

    def __init__(self, v):
        self.v = v

    def item(self):
        return self.v


def reference_statement(label_prefix, epoch, i, n_batches, losses, step_num_targets):
    """CVC-YOLOv3/train.py:81-90 on `losses` (seven objects with .item()) -> the printed statement"""
    loss_labels = ["Total", "L-x", "L-y", "L-w", "L-h", "L-noobj", "L-obj"]
    statement = label_prefix + ' Epoch: ' + str(epoch) + ', Batch: ' + str(i + 1) + '/' + str(n_batches)
    count = 0
    for (loss_label, loss) in zip(loss_labels, losses):
        if count == 0:
            statement += ', Total: ' + '{0:10.6f}'.format(loss.item() / step_num_targets)
            tot_loss = loss.item()
            count += 1
        else:
            statement += ',   ' + loss_label + ': {0:5.2f}'.format(loss.item() / tot_loss * 100) + '%'
    return statement


# rows as the device writes them: seven fp32 losses widened to float, then the count (every value is an fp32 number)
ROWS = {
    "ordinary": [13.708738327026367, 0.5524507164955139, 0.6181793212890625, 0.12075743079185486, 0.09861479699611664,
                 11.921195030212402, 0.3975409269332886, 5.0],
    "one part is nearly all of it": [1000.0009765625, 1000.0, 9.5367431640625e-07, 0.0009765625, 0.0, 0.0, 0.0, 1.0],
    "parts far above the total": [1.401298464324817e-45, 3.4028234663852886e+38, 1.0, 0.5, 0.25, 0.125, 0.0625, 2400.0],
    "no labelled target": [2.5, 0.0, 0.0, 0.0, 0.0, 2.5, 0.0, 0.0],
    "negative total": [-3.0, 1.0, -1.0, 0.5, -0.5, 2.0, -5.0, 3.0],
    "nan total": [float("nan"), 0.25, 0.25, 0.25, 0.25, float("nan"), 0.0, 4.0],
    "inf total": [float("inf"), 1.0, 2.0, 3.0, 4.0, float("inf"), 5.0, 7.0],
}


@pytest.mark.parametrize("name", sorted(ROWS))
@pytest.mark.parametrize("prefix", ["train", "validate"])
def test_step_line_is_the_reference_statement(name, prefix):
    row = ROWS[name]
    want = reference_statement(prefix, 3, 11, 40, [_Item(v) for v in row[:7]], int(row[7]) + 1e-12)
    assert format_step_line(prefix, 3, 11, 40, row) == want
    if name == "nan total":
        assert "nan" in want
    if name == "no labelled target":
        assert "2500000000000.000000" in want            # 2.5 / 1e-12: the reference prints this too


def test_step_line_zero_total_raises_like_the_reference():
    row = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0]
    with pytest.raises(ZeroDivisionError):
        reference_statement("train", 1, 0, 1, [_Item(v) for v in row[:7]], 2 + 1e-12)
    with pytest.raises(ZeroDivisionError):
        format_step_line("train", 1, 0, 1, row)


def reference_rektnet_lines(steps):
    """RektNet/train_eval.py:55-81 on recorded (loc, geo, total) triples -> (descriptions, the Training line)"""
    total_loss = [0, 0, 0]
    batch_num = 0
    descriptions = []
    for loc_loss, geo_loss, loss in steps:
        loc_loss, geo_loss, loss = loc_loss.item(), geo_loss.item(), loss.item()
        descriptions.append(f"Batch {batch_num}. Location Loss: {round(loc_loss,5)}. Geo Loss: {round(geo_loss,5)}. Total Loss: {round(loss,5)}")
        total_loss[0] += loc_loss
        total_loss[1] += geo_loss
        total_loss[2] += loss
        batch_num += 1
    return descriptions, f"\tTraining: MSE/Geometric/Total Loss: {round(total_loss[0]/batch_num,10)}/{round(total_loss[1]/batch_num,10)}/{round(total_loss[2]/batch_num,10)}"


@pytest.mark.parametrize("geo_on_host", [False, True])
def test_rektnet_lines_are_the_reference_statements(geo_on_host):
    steps = [(0.27184075117111206, 0.012345679104328156, 0.2841864228248596), (0.1999969482421875, 1.0000000116860974e-07, 0.19999705255031586),
             (float("nan"), 0.5, float("nan")), (123456.7890625, 0.0, 123456.7890625)]
    if geo_on_host:
        steps = [(a, 0, a) for a, _, _ in steps]                 # CrossRatioLoss without include_geo: torch.tensor(0).item() is the int 0
    want_desc, want_line = reference_rektnet_lines([tuple(_Item(v) for v in s) for s in steps])
    assert [format_batch_description(k, *s) for k, s in enumerate(steps)] == want_desc
    sums = [0, 0, 0]
    for s in steps:
        for j in range(3):
            sums[j] += s[j]
    assert format_epoch_line(sums, len(steps)) == want_line
    if geo_on_host:
        assert "Geo Loss: 0." in want_desc[0] and "/0.0/" in want_line
    with pytest.raises(ZeroDivisionError):
        format_epoch_line([0, 0, 0], 0)


# ---------------------------------------------------------------------------------------------------------------- the ring
class FakeEvent:
    """lands when the test says so; counts what the ring asks of it"""

    def __init__(self, clock, at):
        self.clock, self.at = clock, at
        self.queries = self.syncs = 0

    def query(self):
        self.queries += 1
        return self.clock[0] >= self.at

    def synchronize(self):
        self.syncs += 1
        self.clock[0] = max(self.clock[0], self.at)              # the host has waited until it landed


def drive(ring, steps, lag, drain_every=1):
    """`steps` steps through a RowRing of `ring` slots whose step i lands at time i + lag; the host's clock advances one per step.
    -> (handed-out (step, row, meta) in order, the ring, the events)"""
    clock = [0]
    slots = [None] * ring
    out = []
    r = RowRing(ring, lambda s: slots[s], lambda i, row, meta: out.append((i, row, meta)))
    events = []
    for i in range(steps):
        clock[0] = max(clock[0], i)
        if i % drain_every == 0:
            r.drain()
        s = r.next_slot()
        assert s == i % ring
        assert slots[s] is None or slots[s][0] in [o[1][0] for o in out], "a slot was reused before its row was handed out"
        slots[s] = [float(i), "row of step %d" % i]
        ev = FakeEvent(clock, i + lag)
        events.append(ev)
        r.push(ev, meta=-i)
    return out, r, events, clock


@pytest.mark.parametrize("ring,steps,lag", [(64, 7, 3), (2, 7, 3), (1, 5, 2), (3, 10, 0), (4, 9, 100)])
def test_ring_hands_out_every_row_once_in_step_order(ring, steps, lag):
    out, r, events, clock = drive(ring, steps, lag)
    assert [o[0] for o in out] == list(range(r.head))            # what came out so far: in order, no gaps
    assert r.tail == steps and r.tail - r.head <= ring
    r.drain(block=True)
    assert [o[0] for o in out] == list(range(steps))
    assert [o[1] for o in out] == [[float(i), "row of step %d" % i] for i in range(steps)]
    assert [o[2] for o in out] == [-i for i in range(steps)]
    assert r.head == r.tail == steps and r.drain() == 0


def test_ring_with_room_never_waits_before_the_end():
    out, r, events, clock = drive(64, 7, 3)
    assert r.host_waits == 0 and sum(e.syncs for e in events) == 0
    assert [o[0] for o in out] == [0, 1, 2, 3]                   # steps whose rows had landed by the last drain (time 6, lag 3)
    r.drain(block=True)
    assert r.host_waits == 1 and sum(e.syncs for e in events) == 1 and events[-1].syncs == 1


def test_full_ring_waits_for_the_oldest_row_only():
    out, r, events, clock = drive(2, 7, 3)
    # step i >= 2 finds both slots in flight (lag 3 > ring 2): it waits for step i - 2, which moves the clock to i + 1
    assert r.host_waits == 5 and [e.syncs for e in events] == [1, 1, 1, 1, 1, 0, 0]
    assert [o[0] for o in out] == [0, 1, 2, 3, 4]


def test_late_event_holds_back_later_rows_that_have_landed():
    clock = [0]
    out = []
    r = RowRing(4, lambda s: s, lambda i, row, meta: out.append(i))
    evs = [FakeEvent(clock, 10), FakeEvent(clock, 1), FakeEvent(clock, 1)]
    for e in evs:
        r.next_slot()
        r.push(e)
    clock[0] = 5
    assert r.drain() == 0 and out == []                          # step 0 has not landed: steps 1 and 2 wait behind it
    assert evs[1].queries == 0
    clock[0] = 10
    assert r.drain() == 3 and out == [0, 1, 2]


def test_a_formatter_that_raises_does_not_get_its_row_twice():
    clock = [5]
    seen = []

    def on_row(i, row, meta):
        seen.append(i)
        if i == 1:
            raise ZeroDivisionError("as the reference's statement on a zero total")
    r = RowRing(4, lambda s: s, on_row)
    for _ in range(3):
        r.next_slot()
        r.push(FakeEvent(clock, 0))
    with pytest.raises(ZeroDivisionError):
        r.drain()
    r.drain()
    assert seen == [0, 1, 2]


def test_ring_rejects_nonsense():
    with pytest.raises(ValueError):
        RowRing(0, None, None)
