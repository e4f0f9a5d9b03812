"""The rule the lean f32 kernel's foresight of a runner-up's miss rests on (search_lean.hip), held to a
CPU replay of the two-row pass over the oracle's distances (tests/tools/miss_sim.py): whenever a fresh key of the
candidate c lies below the runner-up p's key, the next pick's candidate is the smallest such key and its runner-up the
second smallest -- or, there being one only, the old p -- unless that entry has left the list.  A change of the list or of the
oracle that breaks the rule fails here, without a GPU.  The hand-made graphs of tests/test_gpu_runner_up_miss.py prove
their miss patterns here too."""
import numpy as np
import pytest

from tests import runner_up_miss as RM


@pytest.fixture(scope="module")
def built_layer0():
    orc, _, _, qs = RM.built()
    return orc, RM.layer0(orc), qs


@pytest.mark.parametrize("ef", RM.EFS)
def test_next_pick_after_a_miss_is_foreseen_from_the_keys(built_layer0, ef):
    orc, adj0, qs = built_layer0
    want_ids, want_d, want_c, _ = orc.search_batch(qs, RM.TOPN, ef, nthreads=8)
    checked = 0
    for qi, q in enumerate(qs):
        sel, _, passes = RM.replay(orc, adj0, q, ef)
        # the replay is the oracle's search: same ids, same distances
        n = int(want_c[qi])
        assert [k[1] for k in sel[:RM.TOPN]] == want_ids[qi, :n].tolist(), (ef, qi)
        assert [np.float32(k[0]) for k in sel[:RM.TOPN]] == want_d[qi, :n].tolist(), (ef, qi)
        assert sum(1 + r["hit"] for r in passes) == _layer0_exp(orc, q, ef), (ef, qi)  # ... same expansions on layer 0
        checked += RM.check_rule(passes, "ef %d query %d" % (ef, qi))
    # the rule was exercised (a list of one entry has no runner-up)
    assert checked > (0 if ef > 1 else -1), (ef, checked)


def _layer0_exp(orc, q, ef):
    e = RM.entry_of(orc, q)[1]
    return int(orc.search_layer(0, q, [e], ef)[2][1])


@pytest.mark.parametrize("name,ef", RM.CASES)
def test_handmade_graphs_provoke_what_their_names_promise(name, ef):
    orc, _, _, qs, g = RM.handmade(name)
    adj0 = {i: g.adj[i] for i in range(RM.N)}
    sel, _, passes = RM.replay(orc, adj0, qs[0], ef)
    dist = orc.distance_batch(qs[0], np.arange(RM.N, dtype=np.uint32))
    assert np.array_equal(dist, g.r)  # distances to q* are the radii, by construction
    want_ids, _, want_c, _ = orc.search_batch(qs[:1], RM.TOPN, ef)
    assert [k[1] for k in sel[:RM.TOPN]] == want_ids[0, :int(want_c[0])].tolist()
    RM.check_rule(passes, "%s ef %d" % (name, ef))
    RM.assert_pattern(name, ef, g, passes, dist)
