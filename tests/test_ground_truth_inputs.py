"""The inputs of tests/test_gpu_ground_truth.py, checked without a GPU: the GPU test CAN fail when the MFMA scan is
wrong (a screen with fewer mantissa bits loses neighbours on the tight families), and it cannot hide a failure by
leaving queries out (at least 0.9 of every precision family's queries are ones the scan must answer exactly).  The
measured shares are recorded in tests/ground_truth_inputs.py and DESIGN.md."""
import numpy as np
import pytest

from oracle import oracle_py as O
from tests import ground_truth_inputs as G


def flat_oracle(X, kind=O.VEC_F32):
    """the oracle over the rows X, no graph: the three calls tests/test_gpu_ground_truth.py makes on the product too"""
    N, d = X.shape
    orc = O.OracleHNSW(8, 16, d, kind)
    orc.import_points(X, np.zeros(N, dtype=np.uint8))
    orc.import_layer(0, np.arange(N, dtype=np.uint32), np.zeros(N + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    orc.set_ep(0)
    return orc


_FAMILY = {}


def family(N, d, offset):
    """(X, Q, oracle ids, oracle distances) of a gauss family, computed once"""
    key = (N, d, offset)
    if key not in _FAMILY:
        X, Q = G.gauss(N, d, offset)
        ids, dist = flat_oracle(X).brute_force(Q, G.K, nthreads=8)
        _FAMILY[key] = (X, Q, ids, dist)
    return _FAMILY[key]


def shares(N, d, offset):
    X, Q, ids, _ = family(N, d, offset)
    return (G.safe(X, Q, G.K, ids).mean(), G.lost(G.screen_emulated(X, Q, G.K, 7), ids).mean(),
            G.lost(G.screen_emulated(X, Q, G.K, 10), ids).mean())


@pytest.mark.parametrize("N,d,offset", G.PRECISION)
def test_cap_most_queries_of_a_precision_family_are_safe(N, d, offset):
    safe, lost7, lost10 = shares(N, d, offset)
    print("gauss(%d, %d, %g): safe %.3f, lost at 7 bits %.3f, at 10 bits %.3f" % (N, d, offset, safe, lost7, lost10))
    assert safe >= G.SAFE_SHARE


def test_no_query_beyond_the_bound_is_safe():
    """the family on which the GPU test asserts only the contract of an unsafe query really is one"""
    safe, lost7, lost10 = shares(*G.BEYOND)
    print("gauss%r: safe %.3f, lost at 7 bits %.3f, at 10 bits %.3f" % (G.BEYOND, safe, lost7, lost10))
    assert safe == 0.0


def test_teeth_a_bf16_screen_fails_at_offset_14():
    assert shares(5000, 128, 14)[1] > 0.0


def test_teeth_a_tf32_screen_fails_at_offset_20():
    assert shares(5000, 128, 20)[2] > 0.0


def test_teeth_at_the_odd_row_width():
    """the tight family of d = 68 catches both lesser screens too (that of d = 768 catches neither: the worst-case
    bound grows with d, a random truncation error with its root -- the table in tests/ground_truth_inputs.py)"""
    assert (9000, 68, 28) in G.PRECISION
    _, lost7, lost10 = shares(9000, 68, 28)
    assert lost7 > 0.0 and lost10 > 0.0


@pytest.mark.parametrize("N,d", [(5000, 128), (9000, 68), (3000, 768)])
def test_centred_rows_cannot_tell_the_screens_apart(N, d):
    """the recorded reason the old check (centred random rows, k + 8 kept) was blind: at offset 0 neither a bf16 nor a
    tf32 screen loses a neighbour on any query"""
    _, lost7, lost10 = shares(N, d, 0)
    assert lost7 == 0.0 and lost10 == 0.0


def test_safe_is_the_stated_predicate():
    """safe() against a direct per-neighbour count on a small tight family"""
    X, Q = G.gauss(400, 16, 150, nq=16)
    ids, _ = flat_oracle(X).brute_force(Q, 5)
    S, E = G.true_scores(X, Q), G.error_bound(X, Q)
    want = [all(np.count_nonzero(S[qi] <= S[qi, x] + 2 * E[qi]) <= 5 + 8 for x in ids[qi]) for qi in range(16)]
    got = G.safe(X, Q, 5, ids)
    assert got.tolist() == want and 0 < sum(want) < 16  # (both outcomes occur)


def test_ints_scores_are_exact_and_tie():
    """every score of an ints family is an integer below 2^24 in magnitude (exact in f32 in any order), and the k-th
    neighbour of every query ties with other points"""
    for N, d, hi in ((300, 380, 3), (5000, 8, 3), (4097, 8, 1), (64, 1272, 3)):
        X, Q = G.ints(N, d, hi)
        S = G.true_scores(X, Q)
        assert np.array_equal(S, np.rint(S)) and np.abs(S).max() < 2 ** 23
        assert ((X.astype(np.float64) ** 2).sum(axis=1) + 2 * np.abs(Q.astype(np.float64) @ X.T.astype(np.float64))).max() < 2 ** 24
    X, Q = G.ints(5000, 8, 3)
    S = np.sort(G.true_scores(X, Q), axis=1)
    assert (S == S[:, G.K - 1:G.K]).sum(axis=1).min() >= 2


def test_dups_repeat_one_row_at_scattered_ids():
    X, Q = G.dups(5000, 64)
    same = np.nonzero((X == X[np.nonzero((X[:, None, 0] == X[None, :, 0]).sum(axis=1) > 1)[0][0]]).all(axis=1))[0]
    assert same.size == 40 and same.max() - same.min() > 2500
    ids, _ = flat_oracle(X).brute_force(Q, G.K)
    assert all(np.array_equal(row, same[:G.K]) or set(row.tolist()) <= set(same.tolist()) for row in ids)


def test_late_rows_beat_a_list_of_ties():
    """the answer of the all-zero query: the six zero rows, then the lowest ids of the ones rows"""
    for N in (300, 5000):
        X, Q = G.late(N, 8)
        zero = np.nonzero((X == 0).all(axis=1))[0]
        assert zero.size == 6 and zero.min() >= 40
        ids, _ = flat_oracle(X).brute_force(Q, G.K)
        assert ids[0].tolist() == zero.tolist() + list(range(G.K - 6))
