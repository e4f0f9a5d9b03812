"""The update machine (tests/update_machine.py) without a GPU: the committed schedules go through every transition the
machine is there for (a condition: the generator is the part that can quietly test nothing); the host half of every
schedule against the real library; and the model's transport rule on literal numbers, so that a mistake in the model
cannot hide one in the product.  The composite schedules (the search-then-post-process entry points) are held to
conditions of their own, by the model alone and by the candidate lists restated over the library's host-built graph,
and a digest pins the committed schedules of seeds 1-3 to what they drew before the composite families existed."""
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


# ---- the composite schedules ----------------------------------------------------------------------------------------
# sha256 (update_machine.digest) of the committed schedules, (seed, cosine) -> digest, taken before the composite
# families were added: seeds 1-3 draw what they drew
DEFAULT_DIGESTS = {
    (1, False): "4efd60940bcb08110289fdf6e0bb9042311cd41e74d0d8486a1d477c67afc781",
    (1, True): "f6869667c1e72f5e3be35748cebfc5aa8119af155cabf44d40c9c8bc26800396",
    (2, False): "a290e486ee61367c30a3f0c8058bacc7a9e86151bbc4f585194b83a12319ed60",
    (2, True): "cc7ebc1f12af699867d920888930b1027618089d7cb1b1538a6a6189a574fae1",
    (3, False): "cc841caca6b6a98250ea47b903e1fb4d71952eb74d440d9a939fc9a72c318a0f",
    (3, True): "05dd23e7cf5f476012dea085f9f504623463ae52b21e03f87a1377f31578c9cd",
}


def test_the_committed_schedules_draw_what_they_drew():
    assert (U.SEEDS, U.STEPS) == ((1, 2, 3), 160)
    for (seed, cosine), want in DEFAULT_DIGESTS.items():
        ops = U.schedule(seed, H.VEC_F32, U.STEPS, cosine)
        assert U.digest(ops) == want, "the schedule of seed %d%s moved" % (seed, " under cosine" if cosine else "")
        assert U.digest(U.schedule(seed, H.VEC_QUANT8, cosine=cosine)) == want  # (the default arguments are these)
        assert not any(op["check"]["family"] in U.COMPOSITE_FAMILIES or "more" in op["check"] for op in ops)


# What the composite schedules have to go through over COMPOSITE_SEEDS, per family: answered twice with nothing deleted
# (the device form, but for the two families whose filter keeps them on the host form) and twice while ids are deleted,
# there on both planned paths; refused once at the host form's limit + 1; answered once on a handle whose deleted count
# came back to 0; once with a row among its candidates or sources that insert_vec patched into the live snapshot; and
# once right after the clone and after the save / load.  (The two anchors: the counts by state, and after clone and load.)
PER_FAMILY = [("state:%s:nodel", 2), ("state:%s:del", 2), ("hpath0:%s", 1), ("hpath1:%s", 1), ("refused:%s", 1),
              ("none_deleted_after_some:%s", 1), ("patched:%s", 1), ("check_after:clone:%s", 1), ("check_after:load:%s", 1)]
# ... and once each: a patched row met while inline_rows is 1 (any family); late: a candidate at or beyond the label
# column's length, a candidate whose label a set_labels changed since the column last went up, with changed words sent by
# this call, and two candidates of different vectors of one query in one document; multi_vec: one id in two lists of a
# query; radius: a query leaving at the first, at a middle and at the last rung of a ladder of three or more, and one
# truncated at max_n
ONCE = ["late:beyond_the_column", "late:label_changed", "late:shared_document", "multi_vec:one_id_in_two_lists",
        "radius:leaves_first", "radius:leaves_middle", "radius:leaves_last", "radius:truncated"]
# the events that are about candidates, said twice: by the model alone (its nearest live rows in float64 are taken for
# candidates) and, with the library's host-built graph at hand, by the restated candidate lists themselves ("seen:")
SEEN_PER_FAMILY = ["patched:%s"]


def composite_events(kind, product):
    ev = collections.Counter()
    for seed in U.COMPOSITE_SEEDS:
        mach = U.Machine(seed, kind, product, families="composite").run()
        assert mach.n_checks == mach.n_expected
        ev.update(mach.m.ev)
    return ev


def missing_events(ev, prefix=""):
    want = [(prefix + t, 1) for t in ONCE] + [(prefix + t % f, 1) for t in SEEN_PER_FAMILY for f in U.COMPOSITE_FAMILIES]
    if not prefix:
        want += [(t % f, n) for t, n in PER_FAMILY for f in U.COMPOSITE_FAMILIES]
        want += [(t % f, n) for t, n in PER_FAMILY for f in U.ANCHORS if t.startswith(("state:", "check_after:"))]
    missing = [t for t, n in want if ev[t] < n]
    if not any(ev[prefix + "patched_inline:%s" % f] for f in U.COMPOSITE_FAMILIES):
        missing.append(prefix + "patched_inline:*")
    return missing


@pytest.mark.parametrize("kind", KINDS)
def test_the_composite_schedules_go_through_every_condition(kind):
    """on the model alone"""
    ev = composite_events(kind, None)
    print({k: ev[k] for k in sorted(ev)})
    missing = missing_events(ev)
    assert not missing, "the composite schedules of seeds %s never reach: %s" % (U.COMPOSITE_SEEDS, missing)
    # the two forced events of their own: every id unmarked and eight ops or more that mark nothing; inline_rows set to
    # 1 between two composite checks
    for seed in U.COMPOSITE_SEEDS:
        ops = U.schedule(seed, kind, families="composite")
        assert len(ops) == U.COMPOSITE_STEPS
        m, quiet = U.Model(U.D), []
        for i, op in enumerate(ops):
            before = int(m.deleted.sum())
            U.apply_op(m, op)
            if op["op"] == "unmark" and before and not m.deleted.any():
                quiet.append(next((j for j in range(i + 1, len(ops)) if ops[j]["op"] in ("mark", "clone")), len(ops)) - i - 1)
        assert max(quiet) >= 8, (seed, quiet)
        flips = [i for i, op in enumerate(ops) if op["op"] == "option" and op.get("key") == "inline_rows" and op["value"] == 1
                 and ops[i - 1]["check"]["family"] in U.COMPOSITE_FAMILIES and op["check"]["family"] in U.COMPOSITE_FAMILIES]
        assert flips, seed


@pytest.mark.parametrize("kind", KINDS)
def test_the_host_half_of_the_composite_schedules_and_what_their_candidates_go_through(kind):
    """every op of the composite schedules on the real library with every GPU call skipped, as above; and, the graph being
    the host's, the restated candidate lists of every composite check: what they go through is counted as seen"""
    ev = composite_events(kind, "host")
    print({k: ev[k] for k in sorted(ev) if k.startswith("seen:")})
    missing = missing_events(ev, "seen:")
    assert not missing, "the candidate lists of the composite schedules of seeds %s never show: %s" % (U.COMPOSITE_SEEDS, missing)


def test_a_composite_failure_names_its_step():
    mach = U.Machine(U.COMPOSITE_SEEDS[0], H.VEC_F32, "host", families="composite")
    step = next(i for i, x in enumerate(mach.ops) if x["op"] == "mark")
    real = mach.m.mark
    mach.m.mark = lambda ids, on: real(ids[:0], on)  # the model loses a deletion
    with pytest.raises(AssertionError) as e:
        mach.run()
    msg = str(e.value)
    assert "seed %d kind %d step %d op [op=mark" % (U.COMPOSITE_SEEDS[0], H.VEC_F32, step) in msg and "check family" in msg, msg


def test_a_composite_schedule_is_drawn_from_its_seed_alone():
    a, b = (U.schedule(U.COMPOSITE_SEEDS[0], H.VEC_F32, families="composite") for _ in range(2))
    assert U.digest(a) == U.digest(b)
    fams = {c["family"] for x in a for c in [x["check"]] + list(x["check"].get("more", ()))}
    assert fams == set(U.COMPOSITE_FAMILIES) | set(U.ANCHORS), fams


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
