"""One merge per committed pass of the lean f32 kernels (search_lean.hip) without a GPU: the hand-made
graphs of tests/one_merge_commit.py prove on a CPU replay over the oracle's distances that their rows provoke the states
their names promise, that merging the keys of c's and p's rows once -- against the bound as it stood before the pass --
leaves the list that two merges leave (asserted inside the replay on every committed pass), and that the replay is the
oracle's search: ids, counts and the three counters, at the ef a graph was laid for and at every other."""
import numpy as np
import pytest

from tests import one_merge_commit as OM
from tests import runner_up_miss as RM

CASES = OM.SCRIPTS + [("overflow", 64), ("overflow", 68)]


def assert_replay_is_the_oracle(kind, ef_laid, ef):
    orc, _, _, qs, _ = OM.handmade(kind, ef_laid)
    sel, counters, _, status = OM.replayed(kind, ef_laid, ef)
    assert status == "ok"
    want_ids, want_d, want_c, want_s = orc.search_batch(qs[:1], OM.TOPN, ef)
    n = int(want_c[0])
    assert n == min(OM.TOPN, len(sel)) and [k[1] for k in sel[:n]] == want_ids[0, :n].tolist(), (kind, ef_laid, ef)
    assert [np.float32(k[0]) for k in sel[:n]] == want_d[0, :n].tolist()
    # (layer 0's counters; the oracle's n_dist has the entry point's distance on top)
    assert [counters[0] + 1, counters[1], counters[2]] == [int(x) for x in want_s[0, :3]], (kind, ef_laid, ef, counters, want_s[0])


@pytest.mark.parametrize("kind,ef", CASES, ids=["%s-%d" % c for c in CASES])
def test_rows_provoke_the_states_their_names_promise(kind, ef):
    OM.assert_states(kind, ef)
    assert_replay_is_the_oracle(kind, ef, ef)


@pytest.mark.parametrize("ef", OM.EFS)
def test_one_merge_is_two_merges_on_every_graph_at_every_ef(ef):
    for kind, ef_laid in CASES:
        if ef_laid != ef:
            assert_replay_is_the_oracle(kind, ef_laid, ef)


def test_one_merge_is_two_merges_on_a_built_index():
    """every committed pass of real walks (tests/runner_up_miss.py's built index)"""
    orc, _, _, qs = RM.built()
    adj0 = RM.layer0(orc)
    folds = cuts = 0
    for ef in (4, 64, 68):
        for q in qs[:24]:
            dist = orc.distance_batch(q, np.arange(len(orc), dtype=np.uint32))
            sel, counters, passes, status = OM.replay(adj0, lambda ids: dist[ids], RM.entry_of(orc, q), ef)
            sel2, counters2, _ = RM.replay(orc, adj0, q, ef)
            assert status == "ok" and sel == sel2 and counters == counters2
            folds += sum(1 for r in passes if r["fold"])
            cuts += "cut" in OM.states(passes)
    assert folds >= 1000 and cuts >= 20, (folds, cuts)


def test_the_three_pass_graphs_are_what_they_promise():
    """full rows: one committed pass with 64 keys below the bound; the visited limit and the NaN graphs: the oracle's
    counters where the walk goes through, its refusal where a distance is NaN"""
    from oracle import oracle_py as O
    q0 = np.zeros((1, OM.D), dtype=np.float32)
    g, orc, _, _ = OM.full_rows()
    adj0 = {i: g.adj[i] for i in range(OM.N)}
    for ef in (64, 65, 68, 128):
        sel, counters, passes, _ = OM.replay(adj0, lambda ids: g.r[ids], RM.entry_of(orc, q0[0]), ef)
        fold = passes[1]
        assert fold["fold"] and len(fold["kc"]) == 32 and len(fold["kp"]) == 32 and fold["last"] == OM.INF
        assert ("cut" in OM.states(passes)) == (ef < 67)
        want = orc.search_batch(q0, OM.TOPN, ef)
        assert [k[1] for k in sel[:OM.TOPN]] == want[0][0].tolist() and [counters[0] + 1, counters[1], counters[2]] == want[3][0].tolist()
    for which, K in OM.VISITED.items():
        g, orc, _, _, want = OM.visited(which)
        s = orc.search_batch(q0, OM.TOPN, 64)[3][0]
        assert s[0] == 1 + K + 2 + 5 + 10 and s[2] == K + 2 + 5 + 10  # (the oracle has no table to overflow)
        assert want is None or want[0] <= s[0]
    for side in ("clean", "c", "p", "both"):
        _, orc, _, _, q, counters = OM.nan_case(side)
        if side == "clean":
            s = orc.search_batch(q, OM.TOPN, 64)[3][0]
            assert [counters[0] + 1, counters[1], counters[2]] == s.tolist()
        else:
            with pytest.raises(O.OracleError) as e:
                orc.search_batch(q, OM.TOPN, 64)
            assert e.value.code == -2
