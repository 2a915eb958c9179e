"""The loaders' hand-over loop (mdcv/data/staging.py `hand_over`) driven by fake `stage` / `enqueue` callables: host scheduling only, no device."""
import threading

from mdcv.data import staging as S

NB = 7


def _run(prefetch, stop_after=None):
    """-> (yielded batches, event log [(what, batch, thread)], {batch: slot stage got}, slots, batches staged ahead at each hand-over)"""
    slots, log, seen, lock = [S.Slot() for _ in range(3)], [], {}, threading.Lock()

    def record(what, j, out):
        with lock:
            log.append((what, j, threading.current_thread()))
        return out

    def stage(j, slot):
        seen[j] = slot
        return record("stage", j, j)
    got, ahead = [], []
    gen = S.hand_over(NB, stage, lambda j: record("enqueue", j, j), slots, prefetch)
    for b in gen:
        got.append(b)
        with lock:
            ahead.append(max(j for what, j, _ in log if what == "stage") - b)
        if b == stop_after:
            gen.close()
    return got, log, seen, slots, ahead


def test_batches_in_order_from_slot_j_mod_3_never_more_than_three_ahead():
    got, log, seen, slots, ahead = _run(True)
    assert got == list(range(NB))
    assert [j for what, j, _ in log if what == "stage"] == list(range(NB)) == [j for what, j, _ in log if what == "enqueue"]
    assert [seen[j] for j in range(NB)] == [slots[j % 3] for j in range(NB)]
    at = {(what, j): i for i, (what, j, _) in enumerate(log)}
    for j in range(NB):
        assert at[("stage", j)] < at[("enqueue", j)]
        if j >= 3:                                               # slot j % 3 is rewritten only after batch j - 3 was handed to enqueue
            assert at[("enqueue", j - 3)] < at[("stage", j)]
    assert all(a <= 3 for a in ahead)
    stagers = {t for what, _, t in log if what == "stage"}
    assert len(stagers) == 1 and threading.current_thread() not in stagers and not stagers.pop().is_alive()
    assert {t for what, _, t in log if what == "enqueue"} == {threading.current_thread()}


def test_an_abandoned_generator_shuts_the_stager_down():
    got, log, _, _, _ = _run(True, stop_after=2)
    staged = [j for what, j, _ in log if what == "stage"]
    assert got == [0, 1, 2] == [j for what, j, _ in log if what == "enqueue"]
    assert staged == list(range(len(staged))) and 3 <= len(staged) <= 5          # 3 and 4 were submitted; 5 and 6 never
    assert not any(t.is_alive() for what, _, t in log if what == "stage")


def test_without_prefetch_stage_runs_inline():
    got, log, seen, slots, ahead = _run(False)
    assert got == list(range(NB)) and ahead == [0] * NB and [seen[j] for j in range(NB)] == [slots[j % 3] for j in range(NB)]
    assert [(what, j) for what, j, _ in log] == [(w, j) for j in range(NB) for w in ("stage", "enqueue")]
    assert {t for _, _, t in log} == {threading.current_thread()}
