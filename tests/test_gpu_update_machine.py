"""The update machine (tests/update_machine.py) on the MI355X: the product and a plain model of its side tables -- the
deleted mask, the label column, the resident mask sets -- driven through the same seeded schedule of inserts, deletions,
label changes, mask set updates, option changes, a clone and a save / load.  After every op one drawn search family is
held to the CPU restatements under the model's predicate (ids, distance bits, counts, counters, status, path), and the
words each HBM copy uploads, the recounts and the compactions to the model's restatement of HbmWords and of the cache
keys.  A failure names seed, kind, step, op, family and query; update_machine.replay(seed, kind, upto) re-runs a prefix.

tests/test_update_machine_host.py holds the committed schedules to the transitions they have to go through."""
import time

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
