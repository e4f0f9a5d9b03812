"""The frontier of the lean f32 kernels' list (search_lean.hip) without a GPU: the hand-made graphs of
tests/frontier.py prove on a CPU replay over the oracle's distances that their rows provoke the states their names
promise (a fixture that stops provoking its state fails here, not silently), and a numpy restatement of the routines --
rank by the ballot below the lane, scatter of ranks 0 .. 3 into four preset places, broadcast; "p is next exactly when no
fresh key of c is below it"; "a and b stay the pair behind p unless a key of c is below min(b, the bound before the
merge)" -- is held to a plain sorted-list replay over random lists with random expanded flags, ties and LK_INVALID
padding included."""
import numpy as np
import pytest

from tests import frontier as FR
from tests import runner_up_miss as RM

CASES = FR.SCRIPTS + [("overflow", 64), ("overflow", 68)]


@pytest.mark.parametrize("kind,ef", CASES, ids=["%s-%d" % c for c in CASES])
def test_rows_provoke_the_states_their_names_promise(kind, ef):
    orc, _, _, qs, g = FR.handmade(kind, ef)
    sel, counters, passes = FR.replayed(kind, ef)
    # the replay with the frontier recorded is the runner-up replay, and that is the oracle's search
    adj0 = {i: g.adj[i] for i in range(FR.N)}
    sel2, counters2, passes2 = RM.replay(orc, adj0, qs[0], ef)
    assert sel == sel2 and counters == counters2
    assert [(r["c"], r["p"], r["hit"]) for r in passes if not r["end"]] == [(r["c"], r["p"], r["hit"]) for r in passes2]
    want_ids, _, want_c, _ = orc.search_batch(qs[:1], FR.TOPN, ef)
    assert [k[1] for k in sel[:FR.TOPN]] == want_ids[0, :int(want_c[0])].tolist()
    FR.assert_states(kind, ef)


def test_rules_hold_on_a_built_index():
    """steps 3 and 4 on every pass of real walks (tests/runner_up_miss.py's built index)"""
    orc, _, _, qs = RM.built()
    adj0 = RM.layer0(orc)
    n3 = n4 = hits = 0
    for ef in (4, 64, 68):
        for q in qs[:24]:
            dist = orc.distance_batch(q, np.arange(len(orc), dtype=np.uint32))
            _, _, passes = FR.replay(adj0, lambda ids: dist[ids], RM.entry_of(orc, q), ef)
            a, b = FR.check_rules(passes, ef)
            n3, n4 = n3 + a, n4 + b
            hits += sum(1 for r in passes if not r["end"] and r["hit"])
    assert n3 >= 1000 and n4 >= 200 and hits > n4, (n3, n4, hits)  # (both arms of step 4 occur)


def key(dist, i, expanded=False):
    bits = np.float32(dist).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | np.uint64(i) | (FR.EXPANDED if expanded else np.uint64(0))


def registers(lst, ef):
    """the list by entry -> the registers of the form that serves ef: [64] or [2, 64], INVALID behind the entries"""
    full = np.full(64 if ef <= 64 else 128, FR.INVALID, dtype=np.uint64)
    full[:len(lst)] = lst
    return full if ef <= 64 else full.reshape(2, 64)


def random_list(rng, ef, n_cur, p_expanded, cut=0):
    """ascending keys with few distinct distances (ties; the ids make every key distinct) and random flags; every
    entry in front of `cut` is expanded"""
    dist = np.sort(rng.integers(1, 9, size=n_cur)).astype(np.float32)
    ids = rng.permutation(1 << 16)[:n_cur]
    keys = np.array(sorted(int(key(d, i)) for d, i in zip(dist, ids)), dtype=np.uint64)
    flag = (rng.random(n_cur) < p_expanded) | (np.arange(n_cur) < cut)
    return keys | np.where(flag, FR.EXPANDED, np.uint64(0))


@pytest.mark.parametrize("seed", range(4))
def test_frontier_is_the_first_four_unexpanded_keys(seed):
    rng = np.random.default_rng(3000 + seed)
    seen = set()
    for trial in range(300):
        ef = int(rng.choice([1, 2, 3, 4, 5, 63, 64, 65, 66, 68, 127, 128]))
        n_cur = int(rng.choice([1, min(2, ef), min(4, ef), max(1, ef // 2), max(1, ef - 1), ef]))
        lst = random_list(rng, ef, n_cur, float(rng.choice([0.0, 0.5, 0.9, 0.97, 1.0])), int(rng.choice([0, 0, 61, 64, 66])))
        want = [k for k in lst if not (k & FR.EXPANDED)][:4]
        got = FR.frontier(registers(lst, ef))
        assert got[:len(want)].tolist() == want and (got[len(want):] == FR.INVALID).all(), (seed, trial, ef, n_cur)
        where = [int(np.nonzero(lst == k)[0][0]) for k in want]
        seen.add(("n", len(want)))
        if where and where[0] >= 64:
            seen.add("tail_only")
        if len(where) > 1 and where[0] < 64 <= where[-1]:
            seen.add("across")
    assert {("n", k) for k in range(5)} | {"tail_only", "across"} <= seen, (seed, seen)


def test_frontier_edges():
    """every place of the only unexpanded entries, alone and in pairs around the head's end; the empty list"""
    for R in (1, 2):
        n = 64 * R
        base = np.array([key(1 + i // 7, 100 + i, True) for i in range(n)], dtype=np.uint64)
        assert (FR.frontier(base.reshape(R, 64) if R == 2 else base) == FR.INVALID).all()
        assert (FR.frontier(np.full((R, 64), FR.INVALID, dtype=np.uint64)) == FR.INVALID).all()
        for i in range(n):
            for j in sorted({i, min(i + 1, n - 1), min(i + 5, n - 1), n - 1}):
                lst = base.copy()
                lst[[i, j]] &= FR.MASK
                want = [lst[i]] + ([lst[j]] if j != i else [])
                got = FR.frontier(lst.reshape(R, 64) if R == 2 else lst)
                assert got[:len(want)].tolist() == want and (got[len(want):] == FR.INVALID).all(), (R, i, j)


@pytest.mark.parametrize("seed", range(4))
def test_commit_and_pair_rules_against_a_sorted_list(seed):
    """c marked, c's keys merged by a plain sorted insert and truncate: p is the first unexpanded entry afterwards
    exactly when the ballot of step 3 is empty, and then the two behind it are a and b whenever step 4 says so"""
    rng = np.random.default_rng(4000 + seed)
    n3 = commons = fallbacks = no_b = 0
    for trial in range(600):
        ef = int(rng.choice([2, 3, 4, 5, 8, 64, 65, 68, 128]))
        n_cur = int(rng.choice([min(2, ef), min(4, ef), max(2, ef - 1), ef, ef]))
        lst = random_list(rng, ef, n_cur, float(rng.choice([0.3, 0.8, 0.95])))
        F = FR.frontier(registers(lst, ef))
        if F[1] == FR.INVALID:
            continue  # no runner-up: nothing to commit
        m = int(rng.choice([0, 1, 1, 2, 3, 6]))
        dist = rng.integers(1, 10, size=m).astype(np.float32)
        fresh = np.array([key(d, i) for d, i in zip(dist, (1 << 16) + rng.permutation(1 << 16)[:m])], dtype=np.uint64)
        keys = np.full(32, FR.INVALID, dtype=np.uint64)  # c's lanes
        keys[rng.permutation(32)[:m]] = fresh
        last = (lst[ef - 1] & FR.MASK) if n_cur >= ef else FR.INVALID
        # the plain replay
        marked = np.where(lst == F[0], lst | FR.EXPANDED, lst)
        merged = np.concatenate([marked, fresh[fresh < last]])
        merged = merged[np.argsort(merged & FR.MASK, kind="stable")][:ef]
        after = [k for k in merged if not (k & FR.EXPANDED)][:3]
        p_next = bool(after) and after[0] == F[1]
        assert FR.commits(keys, F[1]) == p_next, (seed, trial)
        n3 += 1
        if not p_next:
            continue
        pair = after[1:] + [FR.INVALID] * (3 - len(after))
        if FR.pair_stays(keys, F[3], last):
            assert pair == [F[2], F[3]], (seed, trial)
            commons += 1
        else:
            G = FR.frontier(registers(merged, ef))  # the fallback: the frontier of the merged list, p first
            assert G[0] == F[1] and pair == [G[1], G[2]], (seed, trial)
            fallbacks += 1
        no_b += F[3] == FR.INVALID
    assert n3 >= 200 and commons >= 60 and fallbacks >= 30 and no_b >= 20, (seed, n3, commons, fallbacks, no_b)
