"""The big merge of the lean kernels' list (search_lean.hip) without a GPU: the hand-made graphs of
tests/big_merge.py prove on a CPU replay over the oracle's distances that they provoke the merges their names promise
(a fixture that stops provoking its path fails here, not silently), and a numpy restatement of the rank / scatter merge
-- survivors compacted and read back two per trip, shifts, survivor ranks, holes filled in order -- is held to
sorted(list + survivors)[:ef] on the fixtures' merges and on seeded random ones, for lists of one register, head +
tail and four registers."""
import numpy as np
import pytest

from tests import big_merge as BM
from tests import runner_up_miss as RM


@pytest.mark.parametrize("name,ef", BM.PATTERN_CASES)
def test_fixtures_provoke_the_merges_their_names_promise(name, ef):
    key = BM.GRAPHS[name][0]
    orc, _, _, qs, g = BM.handmade(key)
    sel, counters, ms = BM.replayed(key, ef)
    # the replay with its merges recorded is the runner-up replay, and that is the oracle's search
    adj0 = {i: g.adj[i] for i in range(BM.N)}
    sel2, counters2, _ = RM.replay(orc, adj0, qs[0], ef)
    assert sel == sel2 and counters == counters2
    want_ids, _, want_c, _ = orc.search_batch(qs[:1], BM.TOPN, ef)
    assert [k[1] for k in sel[:BM.TOPN]] == want_ids[0, :int(want_c[0])].tolist()
    BM.assert_pattern(name, ef, ms)


def as_registers(before, R):
    lst = np.full(64 * R, BM.INVALID, dtype=np.uint64)
    lst[:len(before)] = before
    return lst


def check_merge(lst, n_cur, keys, ef, what):
    want, n_want = BM.merge_model(lst, n_cur, keys, ef)
    forms = [(1, False)] if ef <= 64 else []
    forms += [(2, True)] if 64 < ef <= 128 else []
    forms += [(4, False)] if ef <= 256 else []
    for R, ht in forms:
        full = np.full(64 * R, BM.INVALID, dtype=np.uint64)
        full[:n_cur] = lst[:n_cur]
        got, n_new = BM.rank_scatter_merge(full, n_cur, keys, ef, R, ht)
        assert n_new == n_want, (what, R, ht)
        assert np.array_equal(got[:n_new], want), (what, R, ht)
        assert (got[n_new:] == BM.INVALID).all(), (what, R, ht)


@pytest.mark.parametrize("key", BM.BUILDERS)
def test_rank_scatter_merge_on_the_fixtures_merges(key):
    checked = 0
    for ef in BM.EFS:
        _, _, ms = BM.replayed(key, ef)
        for i, r in enumerate(BM.big(ms)):
            before = np.array([BM.key_u64(k) for k in r["before"]], dtype=np.uint64)
            # the wave's keys: c's in lanes 0 .. 31, p's in lanes 32 .. 63, the survivors among keys that do not survive
            keys = np.full(64, BM.INVALID, dtype=np.uint64)
            lanes = np.arange(32) + (32 if r["kind"] == "p" else 0)
            sv = np.array([BM.key_u64(k) for k in r["keys"]], dtype=np.uint64)
            keys[np.random.default_rng(i).permutation(lanes)[:len(sv)]] = sv
            check_merge(as_registers(before, 4), r["n_cur"], keys, ef, (key, ef, i))
            checked += 1
    assert checked >= 10, (key, checked)


@pytest.mark.parametrize("seed", range(4))
def test_rank_scatter_merge_on_random_merges(seed):
    rng = np.random.default_rng(1000 + seed)
    checked = 0
    for trial in range(60):
        ef = int(rng.choice([3, 5, 63, 64, 65, 68, 127, 128, 129, 200, 256]))
        n_cur = int(rng.choice([1, min(2, ef), max(1, ef // 2), max(1, ef - 1), ef]))
        m_keys = int(rng.choice([3, 4, 5, 12, 31, 32, 33, 63, 64]))
        # few distinct distances: ties between survivors and with list entries; ids make every key distinct
        dist = rng.integers(1, 40, size=n_cur + m_keys).astype(np.float32)
        ids = rng.permutation(1 << 20)[:n_cur + m_keys]
        allk = (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)
        lst = np.full(256, BM.INVALID, dtype=np.uint64)
        lst[:n_cur] = np.sort(allk[:n_cur])
        keys = np.full(64, BM.INVALID, dtype=np.uint64)
        keys[rng.permutation(64)[:m_keys]] = allk[n_cur:]
        last = lst[ef - 1] if n_cur >= ef else BM.INVALID
        if int((keys < last).sum()) < 3:
            continue
        check_merge(lst, n_cur, keys, ef, (seed, trial, ef, n_cur, m_keys))
        checked += 1
    assert checked >= 30, (seed, checked)
