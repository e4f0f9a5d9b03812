"""The update machine (tests/update_machine.py) on the MI355X: the product and a plain model of its side tables -- the
deleted mask, the label column, the resident mask sets -- driven through the same seeded schedule of inserts, deletions,
label changes, mask set updates, option changes, a clone and a save / load.  After every op one drawn search family is
held to the CPU restatements under the model's predicate (ids, distance bits, counts, counters, status, path), and the
words each HBM copy uploads, the recounts and the compactions to the model's restatement of HbmWords and of the cache
keys.  A failure names seed, kind, step, op, family and query; update_machine.replay(seed, kind, upto) re-runs a prefix.

tests/test_update_machine_host.py holds the committed schedules to the transitions they have to go through."""
import time

import numpy as np
import pytest

import hnsw_rs_amd as H
from tests import update_machine as U

pytestmark = pytest.mark.gpu

KINDS = [H.VEC_QUANT8, H.VEC_F32]
IDS = {H.VEC_QUANT8: "quant8", H.VEC_F32: "f32"}


def run(seed, kind, cosine=False):
    t0 = time.perf_counter()
    mach = U.Machine(seed, kind, "gpu", U.STEPS, cosine).run()
    print("seed %d %s%s: %d ops, %d checks, %.2f s" % (seed, IDS[kind], " cosine" if cosine else "", len(mach.ops),
                                                       mach.n_checks, time.perf_counter() - t0))
    assert mach.n_checks == U.STEPS


@pytest.mark.parametrize("kind", KINDS, ids=IDS.get)
@pytest.mark.parametrize("seed", U.SEEDS)
def test_the_machine(seed, kind):
    run(seed, kind)


@pytest.mark.parametrize("kind", KINDS, ids=IDS.get)
def test_the_machine_under_cosine(kind):
    """metric_cosine set before the first insert (and again on the loaded handle: the file format has no field for it);
    the restatement gets unit rows and unit queries"""
    run(U.SEEDS[0], kind, cosine=True)


# ---- the search-then-post-process entry points: radius, diverse, from_rows / by_id, multi, late -----------------------
# The composite schedules (update_machine.COMPOSITE_SEEDS) run the same ops; their checks hold the five entry points to
# their restatements over candidate lists predicted under the model's predicate and planned path (the host form) or by
# the reference's walk (the device form), the returned stats to the candidates' counters, the upload counters to the
# model and the per-feature counters to the launches of a call.  tests/test_update_machine_host.py holds the schedules
# to what they have to go through.
def run_composite(seed, kind, cosine=False):
    t0 = time.perf_counter()
    mach = U.Machine(seed, kind, "gpu", cosine=cosine, families="composite").run()
    print("composite seed %d %s%s: %d ops, %d checks, %.2f s" % (seed, IDS[kind], " cosine" if cosine else "", len(mach.ops),
                                                                 mach.n_checks, time.perf_counter() - t0))
    assert mach.n_checks == mach.n_expected
    # every composite check of the schedule was held to its restatement, every refused one raised
    checks = [c for op in mach.ops for c in [op["check"]] + list(op["check"].get("more", ()))]
    for fam in U.COMPOSITE_FAMILIES:
        mine = [c for c in checks if c["family"] == fam]
        held, refused = mach.m.ev["held:%s" % fam], mach.m.ev["held_refused:%s" % fam]
        assert (held, refused) == (sum(not c.get("refused") for c in mine), sum(bool(c.get("refused")) for c in mine)), fam
        assert held >= 4 and refused >= 1, (fam, held, refused)


@pytest.mark.parametrize("kind", KINDS, ids=IDS.get)
@pytest.mark.parametrize("seed", U.COMPOSITE_SEEDS)
def test_the_composite_machine(seed, kind):
    run_composite(seed, kind)


@pytest.mark.parametrize("kind", KINDS, ids=IDS.get)
def test_the_composite_machine_under_cosine(kind):
    """as test_the_machine_under_cosine; the rows that from_rows composes are the stored unit rows, composed raw, and the
    cosine option is applied to the composed query as to any other"""
    run_composite(U.COMPOSITE_SEEDS[0], kind, cosine=True)


def prefix_ending_in_an_insert(seed, kind):
    """the first insert_vec step of a composite schedule, past the first steps, after which ids are deleted and the row
    it appends last is live -> the step, that row's id"""
    ops = U.schedule(seed, kind, families="composite")
    for step in range(8, len(ops)):
        if ops[step]["op"] != "insert_vec":
            continue
        m = U.Machine(seed, kind, None, families="composite").run(step + 1).m
        if m.deleted.any() and not m.deleted[m.len - 1]:
            return step, m.len - 1
    raise AssertionError("no such step")


def sensitive_run(check_of, tamper):
    """a prefix of the first composite schedule that ends in an insert_vec, its last check replaced by check_of(row): a
    call that reads the row just appended; the model's view of that row changed by tamper(machine, row) before the run"""
    seed, kind = U.COMPOSITE_SEEDS[0], H.VEC_F32
    step, row = prefix_ending_in_an_insert(seed, kind)
    t0 = time.perf_counter()
    for tampered in (False, True):  # (untouched, the same prefix passes)
        mach = U.Machine(seed, kind, "gpu", families="composite")
        q = mach.ops[step]["vecs"][-1]
        mach.ops[step]["check"] = dict(check_of(row, q), ef=64, exact_max=U.HUGE)  # (the exact path: the row is a candidate)
        if not tampered:
            mach.run(step + 1)
            continue
        tamper(mach, row)
        with pytest.raises(AssertionError) as e:
            mach.run(step + 1)
    print("2 x %d ops, %d checks, %.2f s" % (step + 1, mach.n_checks, time.perf_counter() - t0))
    return str(e.value), "seed %d kind %d step %d op [op=insert_vec" % (seed, kind, step)


def test_the_machine_notices_a_wrong_label_behind_an_insert():
    """the model's label of a row inserted during the prefix is changed; the late check whose vectors are that row fails"""
    def check_of(row, q):
        return {"family": "late", "Q": np.stack([q, q])[None], "mode": 0, "n": 4, "pool": 8}

    def tamper(mach, row):
        mach.tamper_labels[row] = 5  # (the product's: 0, the label of every row inserted since the last set_labels)

    msg, where = sensitive_run(check_of, tamper)
    assert where in msg and "check family late" in msg and "doc_labels differ" in msg, msg


def test_the_machine_notices_one_ulp_in_a_stored_row():
    """one component of a row inserted during the prefix is one ulp up in the rows the model composes from; the from_rows
    check that composes that row alone, and keeps it in its list, fails (its distance to itself is no longer 0)"""
    def check_of(row, q):
        return {"family": "from_rows", "src": np.array([[row]], dtype=np.uint32), "n": 7, "pool": 8, "exclude": False}

    def tamper(mach, row):
        mach.tamper_rows[row] = (3, 1)

    msg, where = sensitive_run(check_of, tamper)
    assert where in msg and "check family from_rows" in msg and "distance bits differ" in msg, msg
