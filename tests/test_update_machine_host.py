"""The update machine (tests/update_machine.py) without a GPU: the committed schedules go through every transition the
machine is there for (a condition: the generator is the part that can quietly test nothing); the host half of every
schedule against the real library; and the model's transport rule on literal numbers, so that a mistake in the model
cannot hide one in the product."""
import collections

import numpy as np
import pytest

import hnsw_rs_amd as H
from tests import update_machine as U

KINDS = [H.VEC_QUANT8, H.VEC_F32]

# what the committed schedules have to go through, at least once (paths: twice) over the seed set
TRANSITIONS = (
    [f"{c}:{o}" for c in ("del", "lab", "set") for o in ("first", "clean", "scatter", "whole")]
    + [f"{c}:grown_within_{d}" for c in ("del", "lab") for d in ("dirty", "clean")]
    + ["del:regrow", "lab:regrow", "del:regrow_clean"]  # grown past capacity (the deleted mask's also with no word listed)
    + ["set:len_passes_allow_bits"]
    + ["row:reused", "row:killed_version", "row:killed_del", "row:killed_len"]
    + ["sort:reused", "sort:killed_version", "sort:killed_del", "sort:killed_len"]
    + ["noop:del", "noop:lab", "noop:set"]
    + ["del:to_zero", "del:back_up", "check_after:clone", "check_after:load"])
TWICE = [f"path0:{f}" for f in U.PATH0_FAMILIES] + [f"path1:{f}" for f in U.PATH1_FAMILIES]


def model_events(kind):
    ev = collections.Counter()
    for seed in U.SEEDS:
        ev.update(U.Machine(seed, kind, None, U.STEPS).run().m.ev)
    return ev


@pytest.mark.parametrize("kind", KINDS)
def test_the_committed_schedules_go_through_every_transition(kind):
    ev = model_events(kind)
    print({k: ev[k] for k in sorted(ev)})
    missing = [t for t in TRANSITIONS if ev[t] < 1] + [t for t in TWICE if ev[t] < 2]
    assert not missing, "the schedules of seeds %s never reach: %s" % (U.SEEDS, missing)


def test_a_schedule_is_drawn_from_its_seed_alone():
    a, b = U.schedule(U.SEEDS[0], H.VEC_F32, U.STEPS), U.schedule(U.SEEDS[0], H.VEC_F32, U.STEPS)
    assert [U.describe(x) for x in a] == [U.describe(x) for x in b]
    assert all(np.array_equal(x["check"].get("Q", 0), y["check"].get("Q", 0)) for x, y in zip(a, b))
    assert len(a) == U.STEPS
    kinds = {x["op"] for s in U.SEEDS for x in U.schedule(s, H.VEC_F32, U.STEPS)}
    assert kinds >= {"insert_vec", "insert_bulk", "mark", "unmark", "set_labels", "set_create", "set_update", "set_write",
                     "set_close", "option", "clone", "save_load"}, kinds
    # one insert opens a new top layer
    for s in U.SEEDS:
        top, opened = -1, 0
        for x in U.schedule(s, H.VEC_F32, U.STEPS):
            if x["op"] in ("insert_vec", "insert_bulk"):
                if x["op"] == "insert_vec" and top >= 0 and int(x["levels"].max()) > top:
                    opened += 1
                top = max(top, int(x["levels"].max()))
        assert opened >= 1, s


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", U.SEEDS)
def test_the_host_half_against_the_library(seed, kind):
    """every op on the real library with every GPU call skipped: is_deleted, deleted_count, deleted_ids, get_labels,
    count_labels_in_ranges, MaskSet.read and MaskSet.count after each op, the parent's independence from a clone and
    equality across save / load"""
    mach = U.Machine(seed, kind, "host", U.STEPS).run()
    assert mach.n_checks == U.STEPS


def test_a_failure_names_its_step():
    """the message of a failing step carries seed, kind, step, op, check family and query"""
    mach = U.Machine(U.SEEDS[0], H.VEC_F32, "host", U.STEPS)
    step = next(i for i, x in enumerate(mach.ops) if x["op"] == "mark")
    real = mach.m.mark
    mach.m.mark = lambda ids, on: real(ids[:0], on)  # the model loses a deletion
    with pytest.raises(AssertionError) as e:
        mach.run()
    msg = str(e.value)
    assert "seed %d kind %d step %d op [op=mark" % (U.SEEDS[0], H.VEC_F32, step) in msg and "check family" in msg, msg


# ---- the transport rule on literal numbers ------------------------------------------------------------------------
def copy_with(nw, slack):
    c = U.Copy("t", collections.Counter())
    assert c.sync(nw, slack) == nw  # no copy yet: whole
    return c


def test_the_whole_copy_threshold_is_exactly_one_eighth():
    c = copy_with(64, 0)
    assert c.cap == 64
    assert c.sync(64, 0) == 0  # nothing changed
    for w in range(8):
        c.touch(w)
    assert c.sync(64, 0) == 8  # dirty x 8 == nw: the eight words are scattered
    for w in range(9):
        c.touch(w)
    assert c.sync(64, 0) == 64  # one more: a whole copy
    c.touch(5)
    c.touch(5)
    assert c.sync(64, 0) == 1  # a word is listed once
    c = copy_with(7, 0)
    c.touch(0)
    assert c.sync(7, 0) == 7  # 1 x 8 > 7
    c = copy_with(8, 0)
    c.touch(3)
    assert c.sync(8, 0) == 1  # 1 x 8 == 8


def test_regrowth_at_d_cap():
    c = copy_with(40, 40 // 8 + 16)  # the deleted mask's slack
    assert c.cap == 61
    assert c.sync(61, 61 // 8 + 16) == 0  # grown to the capacity, nothing listed: nothing travels
    c.touch(60)
    assert c.sync(61, 61 // 8 + 16) == 1 and c.cap == 61
    assert c.sync(62, 62 // 8 + 16) == 62  # one word past it: made afresh, a whole copy, with nothing listed
    assert c.cap == 62 + 7 + 16
    c.touch(1)
    assert c.sync(100, 0) == 100 and c.cap == 100  # ... and with a word listed
    assert copy_with(0, 0).cap == 1  # (a copy of no words still exists)
    ev = c.ev
    assert ev["t:regrow_clean"] == 1 and ev["t:regrow_dirty"] == 1 and ev["t:grown_within_clean"] == 1


def test_an_update_that_changes_nothing_lists_no_word():
    m = U.Model(4)
    m.insert(np.zeros((130, 4), dtype=np.float32), np.zeros(130, dtype=np.uint8))
    m.mark([3, 70], True)
    assert m.del_copy.dirty == {0, 1} and m.del_version == 3 and m.del_nw == 3
    m.mark([3], True)
    m.mark([5], False)
    assert m.del_copy.dirty == {0, 1} and m.del_version == 3 and m.ev["noop:del"] == 2
    m.set_labels([7, 7, 7], [0, 1, 129])
    assert m.lab_copy.dirty == {0, 64} and m.lab_version == 4 and m.lab_nw == 65
    m.set_labels([7], [1])
    assert m.lab_version == 4 and m.ev["noop:lab"] == 1
    m.set_create("A", np.zeros((2, 100), dtype=bool))
    s = m.sets["A"]
    s.update(1, [64, 65], True)
    assert s.copy.dirty == {3} and s.version == [1, 2]
    s.update(1, [64], True)
    s.write(1, s.bits[1].copy())
    assert s.version == [1, 2] and m.ev["noop:set"] == 2
    # the first sync of each: a whole copy, whatever is listed; the second: nothing
    adm, paths, d = m.plan(2, "A", [1, U.NONE], [[U.FULL], [(7, 7)]], exact_max=2)
    assert [int(a.sum()) for a in adm] == [2, 3] and paths == [1, 0]  # ids 64, 65 of row 1; ids 0, 1, 129 are labelled 7
    assert d["deleted_mask_words_uploaded"] == 3 and d["label_words_uploaded"] == 65 and d["mask_set_words_uploaded"] == 4
    assert d["mask_set_recounts"] == 1 and d["mask_set_compactions"] == 1 and d["uploads"] == 1
    adm, paths, d = m.plan(2, "A", [1, U.NONE], [[U.FULL], [(7, 7)]], exact_max=2)
    assert d == U.zero_delta()
