"""The small merge of the lean kernels' list (search_lean.hip) without a GPU: the hand-made graphs of
tests/small_merge.py prove on a CPU replay over the oracle's distances that every row provokes the merge its name
promises (a fixture that stops provoking its path fails here, not silently), and a numpy restatement of the insertion
-- a compare mask, the mask of the entries before, two selects; the head's last entry carried to the tail's front; no
test against the bound between two keys; one cut at ef -- is held to a plain sorted insert and truncate: exhaustively on
lists of up to six entries with up to two survivors, and on seeded random lists at the real widths, for lists of one
register, head + tail and four, five and eight registers, expanded flags and invalid padding included."""
import itertools

import numpy as np
import pytest

from tests import runner_up_miss as RM
from tests import small_merge as SM


@pytest.mark.parametrize("ef", SM.EFS)
def test_rows_provoke_the_merges_their_names_promise(ef):
    orc, _, _, qs, s = SM.handmade(ef)
    sel, counters, ms = SM.replayed(ef)
    # the replay with its merges recorded is the runner-up replay, and that is the oracle's search
    adj0 = {i: s.g.adj[i] for i in range(SM.N)}
    sel2, counters2, _ = RM.replay(orc, adj0, qs[0], ef)
    assert sel == sel2 and counters == counters2
    want_ids, _, want_c, _ = orc.search_batch(qs[:1], SM.TOPN, ef)
    assert [k[1] for k in sel[:SM.TOPN]] == want_ids[0, :int(want_c[0])].tolist()
    SM.assert_pattern(ef, ms, s)
    # the script's own model of the walk is the replay: its list is the replay's when the last row has been merged
    if len(ms) > len(s.names):
        assert s.cur == ms[len(s.names)]["before"]


def key(v, i, expanded=False):
    return (np.uint64(v) << np.uint64(32)) | np.uint64(i) | (SM.EXPANDED if expanded else np.uint64(0))


def check(lst, n_cur, keys, ef, what, min_forms=1):
    """every list form that serves ef: the restatement against the sorted insert and truncate"""
    want, n_want = SM.merge_model(lst, n_cur, keys, ef)
    fs = SM.forms(ef)
    assert len(fs) >= min_forms
    for R, ht in fs:
        full = np.full(64 * R, SM.INVALID, dtype=np.uint64)
        full[:n_cur] = lst[:n_cur]
        got, n_new, bound = SM.small_merge(full, n_cur, keys, ef, R, ht)
        assert n_new == n_want, (what, R, ht)
        assert np.array_equal(got[:n_new], want), (what, R, ht, got[:n_new], want)
        assert (got[n_new:] == SM.INVALID).all(), (what, R, ht)
        assert bound == ((want[ef - 1] & SM.MASK) if n_want >= ef else SM.INVALID), (what, R, ht)


@pytest.mark.parametrize("ef", range(1, 7))
def test_exhaustive_small_lists(ef):
    """lists of 0 .. min(ef, 6) entries at the even values, one or two keys at every pair of odd values (in front of,
    between and behind the entries, below the bound or not), in either lane order, flags on every other entry or none"""
    checked = 0
    for n_cur in range(0, ef + 1):
        for flags in (False, True):
            lst = np.array([key(2 * (i + 1), 100 + i, flags and i % 2 == 0) for i in range(n_cur)], dtype=np.uint64)
            odd = range(1, 2 * n_cur + 4, 2)
            for pair in itertools.chain(((a,) for a in odd), itertools.permutations(odd, 2)):
                keys = np.full(64, SM.INVALID, dtype=np.uint64)
                for lane, v in zip((5, 40), pair):
                    keys[lane] = key(v, 200 + v)
                check(lst, n_cur, keys, ef, (ef, n_cur, flags, pair), min_forms=4)
                checked += 1
    assert checked >= 20


@pytest.mark.parametrize("ef", range(65, 71))
def test_exhaustive_around_the_heads_end(ef):
    """head + tail: full and nearly full lists, one or two keys at every place from entry 60 on, and in front"""
    checked = 0
    for n_cur in range(max(62, ef - 3), ef + 1):
        lst = np.array([key(2 * (i + 1), 100 + i, i % 3 == 0) for i in range(n_cur)], dtype=np.uint64)
        odd = [1] + list(range(121, 2 * n_cur + 4, 2))
        for pair in itertools.chain(((a,) for a in odd), itertools.permutations(odd, 2)):
            keys = np.full(64, SM.INVALID, dtype=np.uint64)
            for lane, v in zip((33, 62), pair):
                keys[lane] = key(v, 200 + v)
            check(lst, n_cur, keys, ef, (ef, n_cur, pair), min_forms=4)
            checked += 1
    assert checked >= 100


@pytest.mark.parametrize("seed", range(4))
def test_random_lists_at_the_real_widths(seed):
    rng = np.random.default_rng(2000 + seed)
    checked = 0
    for trial in range(120):
        ef = int(rng.choice([1, 2, 3, 63, 64, 65, 68, 127, 128, 129, 200, 256, 257, 320, 321, 512]))
        n_cur = int(rng.choice([1, min(2, ef), max(1, ef // 2), max(1, ef - 1), ef, ef]))
        m_keys = int(rng.choice([1, 2, 2, 3, 5]))  # keys in the wave: at most two of them may survive
        # few distinct distances: ties between survivors and with list entries; ids make every key distinct
        dist = rng.integers(1, 12, size=n_cur + m_keys).astype(np.float32)
        ids = rng.permutation(1 << 20)[:n_cur + m_keys]
        allk = (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)
        lst = np.sort(allk[:n_cur])
        lst = lst | np.where(rng.random(n_cur) < 0.5, SM.EXPANDED, np.uint64(0))
        keys = np.full(64, SM.INVALID, dtype=np.uint64)
        keys[rng.permutation(64)[:m_keys]] = allk[n_cur:]
        last = (lst[ef - 1] & SM.MASK) if n_cur >= ef else SM.INVALID
        if not 1 <= int((keys < last).sum()) <= 2:
            continue
        check(lst, n_cur, keys, ef, (seed, trial, ef, n_cur, m_keys))
        checked += 1
    assert checked >= 40, (seed, checked)


@pytest.mark.parametrize("ef", SM.EFS)
def test_restatement_on_the_fixtures_merges(ef):
    """every one- and two-survivor merge of the fixture's replay, the survivors in c's lanes or in p's"""
    _, _, ms = SM.replayed(ef)
    checked = 0
    for i, r in enumerate(ms):
        if not 1 <= r["m"] <= 2:
            continue
        lst = np.array([SM.BM.key_u64(k) for k in r["before"]], dtype=np.uint64)
        keys = np.full(64, SM.INVALID, dtype=np.uint64)
        lanes = np.arange(32) + (32 if r["kind"] == "p" else 0)
        keys[np.random.default_rng(i).permutation(lanes)[:r["m"]]] = [SM.BM.key_u64(k) for k in r["keys"]]
        check(lst, r["n_cur"], keys, ef, (ef, i))
        checked += 1
    assert checked >= 7, (ef, checked)  # ef 1 has seven rows of one or two survivors, every other ef more
