"""No GPU: the schedule-hazard analysis and its extent table on their own (tests/helpers/sched_hazards.py).

Synthetic traces are plain lists of the records the recorder writes.  They pin down what the vector clocks take for ordered -- forks, the
fork-on-dispatch arm / wait pair, re-recorded events, three streams joined through events as the pipelined optimizer joins them -- and what the
strided sets take for overlapping; the table checks make sure that an entry point added to include/mdcv_hip.h later cannot escape the model.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sched_hazards as sh  # noqa: E402

MAIN, SIDE, PAR = 0x10, 0x20, 0x30
BUF = 0x1000                       # one allocation of 4096 bytes, another behind it
ALLOCS = [("buf", BUF, 4096), ("other", 0x4000, 4096)]


def launch(name, stream, *acc):
    """acc: (mode, ptr, bytes) contiguous ranges"""
    return dict(op="launch", name=name, stream=stream, acc=[(f"a{i}", p, 1, n, n, m) for i, (m, p, n) in enumerate(acc)])


def fork(src, dst):
    return dict(op="fork", src=src, dst=dst)


def hazards(trace):
    res = sh.analyse(trace, ALLOCS)
    assert not res.violations, res.violations
    return res.findings


def test_ordered_fork_chain_is_clean():
    t = [launch("produce", MAIN, ("w", BUF, 256)), fork(MAIN, SIDE), launch("consume", SIDE, ("r", BUF, 256), ("w", BUF + 1024, 64)),
         fork(SIDE, PAR), launch("third", PAR, ("rw", BUF + 1024, 64), ("w", BUF, 256)), fork(PAR, MAIN), launch("again", MAIN, ("w", BUF, 4096))]
    res = sh.analyse(t, ALLOCS)
    assert res.findings == [] and res.violations == []
    assert res.launches == 4 and res.streams == 3 and res.forks == 3 and res.cross_pairs > 0


CASES = {"RAW": (("w", BUF + 64, 128), ("r", BUF + 128, 128), (BUF + 128, BUF + 192)),
         "WAR": (("r", BUF, 512), ("w", BUF + 500, 100), (BUF + 500, BUF + 512)),
         "WAW": (("rw", BUF + 8, 8), ("w", BUF, 1024), (BUF + 8, BUF + 16))}


@pytest.mark.parametrize("kind", sorted(CASES))
def test_unordered_conflict_is_reported_once_with_its_range(kind):
    first, second, (lo, hi) = CASES[kind]
    t = [launch("first", MAIN, first, ("r", 0x4000, 64)), launch("bystander", MAIN, ("r", BUF + 2048, 8)),
         launch("second", SIDE, second, ("r", 0x4000, 64))]
    f = hazards(t)
    assert len(f) == 1, f
    f = f[0]
    assert (f.kind, f.earlier["name"], f.later["name"], f.buffer) == ("hazard", "first", "second", "buf")
    assert (f.lo + BUF, f.hi + BUF) == (lo, hi) and f.label.startswith(kind)
    assert (f.earlier["stream"], f.later["stream"]) == (MAIN, SIDE)


@pytest.mark.parametrize("kind", sorted(CASES))
def test_fork_between_orders_the_conflict(kind):
    first, second, _ = CASES[kind]
    t = [launch("first", MAIN, first), fork(MAIN, SIDE), launch("second", SIDE, second)]
    res = sh.analyse(t, ALLOCS)
    assert res.findings == [] and res.cross_pairs == 1


def test_fork_in_the_wrong_direction_orders_nothing():
    t = [launch("first", MAIN, ("w", BUF, 64)), fork(SIDE, MAIN), launch("second", SIDE, ("r", BUF, 64))]
    f = hazards(t)
    assert len(f) == 1 and (f[0].earlier["name"], f[0].later["name"]) == ("first", "second")


def test_fork_covers_only_what_was_enqueued_before_it():
    t = [launch("a", MAIN, ("w", BUF, 64)), fork(MAIN, SIDE), launch("b", MAIN, ("w", BUF + 64, 64)), launch("c", SIDE, ("r", BUF, 128))]
    f = hazards(t)
    assert len(f) == 1 and (f[0].earlier["name"], f[0].later["name"]) == ("b", "c") and (f[0].lo, f[0].hi) == (64, 128)


def test_arm_orders_up_to_and_including_the_armed_launch_only():
    ev = ("ring", 1)
    t = [launch("before", MAIN, ("w", BUF, 64)), dict(op="arm", src=MAIN, ev=ev), launch("armed", MAIN, ("w", BUF + 64, 64)),
         launch("after", MAIN, ("w", BUF + 128, 64)), dict(op="fwait", dst=SIDE, ev=ev), launch("reader", SIDE, ("r", BUF, 192))]
    res = sh.analyse(t, ALLOCS)
    assert res.violations == [] and res.arms == 1
    assert [(f.earlier["name"], f.later["name"], f.lo, f.hi) for f in res.findings] == [("after", "reader", 128, 192)]


def test_arm_followed_by_a_launch_on_another_stream_is_flagged():
    ev = ("ring", 1)
    t = [launch("producer", MAIN, ("w", BUF, 64)), dict(op="arm", src=MAIN, ev=ev), launch("elsewhere", PAR, ("w", 0x4000, 8)),
         dict(op="fwait", dst=SIDE, ev=ev), launch("reader", SIDE, ("r", BUF, 64))]
    res = sh.analyse(t, ALLOCS)
    assert [v.kind for v in res.violations] == ["arm-wrong-stream"] and res.violations[0].later["name"] == "elsewhere"
    assert [(f.earlier["name"], f.later["name"]) for f in res.findings] == [("producer", "reader")]      # and nothing was ordered by it


def test_torch_side_work_does_not_take_the_armed_event():
    ev = ("ring", 1)
    memset = launch("_zero_tensor", PAR, ("w", 0x4000, 8))
    memset["torch"] = True
    t = [dict(op="arm", src=MAIN, ev=ev), memset, launch("armed", MAIN, ("w", BUF, 64)), dict(op="fwait", dst=SIDE, ev=ev),
         launch("reader", SIDE, ("r", BUF, 64))]
    res = sh.analyse(t, ALLOCS)
    assert res.violations == [] and res.findings == []


def test_wait_before_the_armed_call_and_wait_on_an_unknown_event_are_flagged():
    ev = ("ring", 1)
    res = sh.analyse([dict(op="arm", src=MAIN, ev=ev), dict(op="fwait", dst=SIDE, ev=ev), launch("late", MAIN, ("w", BUF, 8))], ALLOCS)
    assert [v.kind for v in res.violations] == ["wait-before-call"]
    res = sh.analyse([dict(op="fwait", dst=SIDE, ev=("ring", 9)), dict(op="wait", stream=SIDE, ev=("torch", 5))], ALLOCS)
    assert [v.kind for v in res.violations] == ["wait-unrecorded", "wait-unrecorded"]


def test_a_wait_sees_the_record_that_preceded_it_not_a_later_one():
    ev = ("torch", 1)
    t = [launch("w1", MAIN, ("w", BUF, 64)), dict(op="record", stream=MAIN, ev=ev), launch("w2", MAIN, ("w", BUF + 64, 64)),
         dict(op="wait", stream=SIDE, ev=ev), dict(op="record", stream=MAIN, ev=ev), launch("reader", SIDE, ("r", BUF, 128))]
    f = hazards(t)
    assert [(x.earlier["name"], x.later["name"]) for x in f] == [("w2", "reader")]
    t.insert(5, dict(op="wait", stream=SIDE, ev=ev))         # a wait behind the second record does see w2
    assert hazards(t) == []


def test_three_streams_joined_through_events_as_the_pipelined_optimizer_joins_them():
    """main: backward writes g -> param stream (wait_stream): update reads g, writes p, record ev -> main: forward waits ev, reads p"""
    g, p, ev = BUF, BUF + 1024, ("torch", 7)
    good = [launch("bwd", MAIN, ("w", g, 512)), fork(MAIN, PAR), launch("update", PAR, ("r", g, 512), ("rw", p, 512)),
            dict(op="record", stream=PAR, ev=ev), dict(op="wait", stream=MAIN, ev=ev), launch("fwd", MAIN, ("r", p, 512)),
            launch("bwd2", MAIN, ("w", g, 512))]
    res = sh.analyse(good, ALLOCS)
    assert res.findings == [] and res.violations == [] and res.cross_pairs == 3
    late = [r for r in good if r.get("op") != "wait"]        # the forward does not wait: it reads p under the update, and bwd2 rewrites g
    f = hazards(late)
    assert [(x.earlier["name"], x.later["name"], x.label[:3]) for x in f] == [("update", "fwd", "RAW"), ("update", "bwd2", "WAR")]


def test_same_stream_is_never_a_finding_and_two_reads_never_conflict():
    t = [launch("a", MAIN, ("w", BUF, 64)), launch("b", MAIN, ("rw", BUF, 64)), launch("c", SIDE, ("r", BUF + 512, 64)),
         launch("d", PAR, ("r", BUF + 512, 64))]
    res = sh.analyse(t, ALLOCS)
    assert res.findings == [] and res.cross_pairs == 0


def test_pointer_outside_every_allocation_is_a_finding():
    res = sh.analyse([launch("stray", MAIN, ("w", 0x9000, 8)), launch("overrun", MAIN, ("w", BUF + 4090, 8))], ALLOCS)
    assert [f.kind for f in res.findings] == ["unresolved", "unresolved"] and "runs past the end" in res.findings[1].text


# ------------------------------------------------------------------------------------------------ strided sets
def test_channel_slices_of_one_buffer():
    pitch = 256                                              # 128 bf16 channels per pixel row
    a = sh.rows(BUF, 10, 128, 64, 2)                         # channels 0..63
    b = sh.rows(BUF + 128, 10, 128, 64, 2)                   # channels 64..127
    c = sh.rows(BUF + 96, 10, 128, 40, 2)                    # channels 48..87: shares with both
    assert a == (BUF, 10, pitch, 128)
    assert sh.overlap(a, b, BUF) is None and sh.overlap(b, a, BUF) is None
    assert sh.overlap(a, c, BUF) is not None and sh.overlap(c, b, BUF) is not None
    assert sh.overlap(a, sh.flat(BUF + 128, 128), BUF) is None            # one row takes the other's pitch: bytes 128..255 of row 0
    assert sh.overlap(a, sh.flat(BUF + 120, 16), BUF) == (BUF + 120, BUF + 136)
    d = sh.rows(BUF + 128, 10, 96, 32, 2)                    # another pitch: hulls decide
    assert sh.overlap(a, d, BUF) == (BUF + 128, min(sh.hull(a)[1], sh.hull(d)[1]))
    assert sh.overlap(a, sh.rows(BUF + 4096, 4, 128, 64, 2), BUF) is None  # disjoint hulls
    t = [dict(op="launch", name="left", stream=MAIN, acc=[("o", *a, "w")]), dict(op="launch", name="right", stream=SIDE, acc=[("o", *b, "w")]),
         dict(op="launch", name="middle", stream=PAR, acc=[("o", *c, "r")])]
    f = sh.analyse(t, ALLOCS).findings
    assert sorted((x.earlier["name"], x.later["name"]) for x in f) == [("left", "middle"), ("right", "middle")]


def test_empty_and_null_sets_vanish():
    assert sh.flat(0, 64) is None and sh.flat(None, 64) is None and sh.flat(BUF, 0) is None and sh.rows(BUF, 0, 8, 8, 2) is None


# ------------------------------------------------------------------------------------------------ the table against the header
DIRECTIONS = sh.parse_directions()


def test_every_stream_entry_has_an_extent_row_or_a_reason():
    entries = sh.stream_entries(DIRECTIONS)
    assert len(entries) > 80 and "conv2d" in entries and "stream_fork" not in entries
    for n in entries:
        assert (n in sh.TABLE) != (n in sh.NOT_IN_PLANS), f"mdcv_{n} takes a stream: give it an extent row in TABLE or a reason in NOT_IN_PLANS (not both)"
    for n, why in sh.NOT_IN_PLANS.items():
        assert n in entries and len(why) > 20, n
    assert set(sh.TABLE) <= set(entries)
    for n in sh.SYNC_ENTRIES:
        assert n in DIRECTIONS


def test_no_const_pointer_is_declared_written_and_every_pointer_has_an_extent():
    for n, row in sh.TABLE.items():
        spec = {a[0]: a for a in DIRECTIONS[n]}
        ptrs = [a[0] for a in DIRECTIONS[n] if a[1] and a[0] != "stream"]
        for w in row.get("wo", ()):
            assert w in spec and spec[w][1] and not spec[w][2], f"mdcv_{n}: {w} is declared write-only but is const (or no pointer) in the header"
        assert sorted(row["ptrs"]) == sorted(ptrs), f"mdcv_{n}: extents {sorted(row['ptrs'])} against pointers {sorted(ptrs)}"
        assert set(row) <= {"ptrs", "wo", "indirect"}, n       # (no "to the end of the allocation" extents: there is no such key)


def test_header_directions_keep_const():
    assert ("partial", True, False) in DIRECTIONS["bn_stats_finalize"] and ("partial", True, False) in DIRECTIONS["bn_bwd_finalize_rows"]   # folded in place
    d = {a[0]: a for a in DIRECTIONS["conv2d_wgrad"]}
    assert d["dy"] == ("dy", True, True) and d["ws"] == ("ws", True, False) and d["splits"] == ("splits", False, False)
    assert ("losses", True, True) in DIRECTIONS["train_log_step"]


class _Sizes:
    """stand-in for the library's size queries"""

    @staticmethod
    def conv2d_stats_rows_geom(*a):
        return 5

    @staticmethod
    def pw_bwd_slabs(*a):
        return 3


def test_accesses_take_direction_from_the_header_and_extent_from_the_table():
    q = sh.Queries(_Sizes, None)
    #        dtype mode in     ldc w       out    ldc bias addsrc ldc stats  B  Hi Wi Ci  Ho Wo No  KH KW s  p  d
    args = (1, 0, 0x1000, 16, 0x2000, 0x3000, 64, None, 0x3040, 64, 0x5000, 2, 4, 4, 16, 4, 4, 32, 3, 3, 1, 1, 1, None)
    acc = {a[0]: a[1:] for a in sh.accesses_of(DIRECTIONS, "conv2d", args, q)}
    assert acc["in"] == (0x1000, 32, 32, 32, "r") and acc["w_packed"] == (0x2000, 1, 2 * 32 * 9 * 16, 2 * 32 * 9 * 16, "r")
    assert acc["out"] == (0x3000, 32, 128, 64, "w") and acc["addsrc"] == (0x3040, 32, 128, 64, "r")
    assert acc["stats_partial"] == (0x5000, 1, 5 * 2 * 32 * 4, 5 * 2 * 32 * 4, "w") and "bias" not in acc
    assert sh.overlap(acc["out"][:4], acc["addsrc"][:4], 0x3000) is None          # the two channel halves of one concat buffer
    args = (1, 0x100, 8, 0x200, 8, 0x300, 0x400, 8, None, 0, 0x500, 3, None, 0, None, None, None, 0, 0.0, None, 10, 64, 128, None)
    acc = {a[0]: a[1:] for a in sh.accesses_of(DIRECTIONS, "pw_bwd", args, q)}
    assert acc["ws"] == (0x500, 1, 4 * 3 * 128 * 64, 4 * 3 * 128 * 64, "w") and acc["dx"][4] == "w" and acc["dy"][4] == "r"
    assert set(acc) == {"dy", "x", "wd_packed", "dx", "ws"}


def test_pack_table_rows_are_decoded():
    import struct
    rec = struct.pack("<QQQiiiiiiiiQQ", 0x100, 0x200, 0x300, 30, 12, 9, 32, 16, 0, 0, 0, 0x400, 0x500) + \
        struct.pack("<QQQiiiiiiiiQQ", 0x600, 0x700, 0, 8, 8, 1, 8, 8, 0, 0, 0, 0, 0)
    q = sh.Queries(None, lambda p, n: rec[p - 0x9000:p - 0x9000 + n])
    acc = sh.accesses_of(DIRECTIONS, "pack_weights_batched", (1, 0x9000, 2, 9, None), q)
    got = {a[0]: a[1:] for a in acc}
    assert got["table"] == (0x9000, 1, 144, 144, "r")
    assert got["table[0].w_oihw"] == (0x100, 1, 4 * 30 * 12 * 9, 4 * 30 * 12 * 9, "r") and got["table[0].w_fwd"][-1] == "w"
    assert got["table[0].w_dgrad"] == (0x300, 1, 2 * 32 * 9 * 16, 2 * 32 * 9 * 16, "w") and got["table[0].bias_padded"] == (0x500, 1, 128, 128, "w")
    assert "table[1].w_dgrad" not in got and "table[1].bias" not in got and "table[1].bias_padded" not in got
    acc = sh.accesses_of(DIRECTIONS, "pack_weights_batched", (1, 0x9000 + 72, 1, 9, None), q)      # a parameter group's slice of the table
    assert {a[0] for a in acc} == {"table", "table[0].w_oihw", "table[0].w_fwd"}
