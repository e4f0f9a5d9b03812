"""Inputs that pin the two exhaustive scans (hnsw_brute_force, hnsw_brute_force_fast) to the oracle, and the float64
predicate that says when the MFMA scan MUST equal the oracle bit for bit.  numpy only: no GPU, no product, no oracle.

Families (rows X and queries Q, float32, seeded with np.random.default_rng):

  gauss(N, d, offset)  standard normal plus a common offset, rows and queries alike.  The offset grows every norm and
                       dot product (and with them the rounding error of a score) without changing the distances between
                       points: it is the knob that brings the score gaps down to the rounding bound.
  ints(N, d, hi)       integers in [0, hi] with d hi^2 < 2^22: every product, norm, score and squared distance is exact
                       in f32, distinct squared distances have distinct f32 square roots, so the screen's (score, id)
                       order IS the exact (dist, id) order -- with massive ties.  The MFMA scan must equal the exact
                       answer on every query; no bound is needed.
  dups(N, d)           gauss(N, d, 0) with one row repeated 40 times at scattered ids; a query is that row plus small
                       noise.  Equal rows get bit-equal scores (same norm, same dot product in the same order), the
                       (score, id) order keeps the lowest ids, and the answer must equal the exact scan's.
  late(N, d)           rows of ones, six rows of zeros at scattered ids from 40 on; queries of zeros and ones.  For a
                       query nearer to the zero rows the answer is those six and then the LOWEST ids of the ones rows,
                       which all tie -- but every lane of the screen has filled its list with tied rows before a better
                       row arrives, and must then give up the tied row of the HIGHEST id.  Scores are exact, as in ints.

safe(X, Q, k, oracle_ids) -> bool per query.  The screen ranks points by the score s(x) = |x|^2 - 2 x.q (the query's
own norm does not change the order), computed in f32: the norm by one left-to-right chain, the dot product by the
matrix cores in an order of their own, then one subtraction.  With u = 2^-24, for ANY summation order and any fusing of
multiply and add,

    |computed norm - |x|^2|          <= gamma_d |x|^2               (d products, d - 1 additions)
    |computed dot  - x.q|            <= gamma_d sum |x_i| |q_i|
    |computed s    - s|              <= u (|x|^2 + 2 sum|x_i||q_i|) + (1 + u) gamma_d (|x|^2 + 2 sum|x_i||q_i|)

(gamma_d = d u / (1 - d u); doubling the dot product is exact), so with

    E_q = 1.01 (d + 2) 2^-24 max_x (|x|^2 + 2 sum_i |x_i| |q_i|)

every computed score of query q is within E_q of the true one (1.01 absorbs the second-order terms for d u < 0.005, i.e.
d < 80000).  Nothing is assumed about the matrix core's internal order.  A query is SAFE if for every id x in the
oracle's top k at most k + 8 points y (x included) have s(y) <= s(x) + 2 E_q.  For a safe query the screen's k + 8
contains the oracle's whole top k: were x pushed out, k + 8 OTHER points would have a computed score no greater than
x's, hence a true score within 2 E_q of it, and the predicate allows at most k + 7 others.  The re-rank then computes
the reference's own distances of a superset of the oracle's top k and sorts by (dist, id): ids and distance bits must be
the oracle's.  tests/test_gpu_ground_truth.py asserts exactly that, and asserts the share of safe queries itself.

screen_emulated(X, Q, k, mantissa_bits): the k + 8 best ids by (score, id), the dot product of the score computed
(float64) from rows and queries truncated to that many mantissa bits, the norm from the full f32 row (the norm kernel is
a kernel of its own) -- what a screen would keep whose matrix instruction read bf16 (7 bits) or tf32 (10 bits)
operands.  lost(...) says per query whether such a screen dropped one of the oracle's top k.

Measured (tests/test_ground_truth_inputs.py asserts the conditions; k = 12, 64 queries, seed 1; `lost` = share of
queries on which the emulated screen loses at least one of the oracle's neighbours):

    family                  safe share   smallest margin (gap / 2 E)   lost at 7 bits   lost at 10 bits
    gauss(5000, 128, 0)     1.000        254                           0.000            0.000
    gauss(5000, 128, 14)    1.000        1.31                          0.812            0.000
    gauss(5000, 128, 20)    0.922        0.65                          1.000            0.125
    gauss(9000, 68, 0)      1.000        515                           0.000            0.000
    gauss(9000, 68, 28)     0.953        0.71                          1.000            0.422
    gauss(3000, 768, 0)     1.000        31.8                          0.000            0.000
    gauss(3000, 768, 5)     1.000        1.04                          0.000            0.000
    gauss(5000, 128, 100)   0.000        0.03                          1.000            1.000

At offset 0 (the centred rows of every earlier check) the gaps are 30 to 500 times the bound and neither lesser screen
loses anything: such rows cannot tell the f32 matrix instruction from a bf16 one.  At d = 768 the worst-case bound
(linear in d) reaches the gaps at offset 5, where a random truncation error (root of d) does not yet: that family has no
teeth against a lesser screen and is kept for the width alone; at offset 6 its safe share is 0.859, under the cap.
"""
import numpy as np

K = 12          # the k of the MFMA cases (the host serves k <= 12: k + 8 <= the 20 candidates a lane keeps)
SCREEN = 8      # the screen keeps k + 8
PAD = 0xFFFFFFFF

# the gauss families the GPU test asserts exactness on: (N, d, offset); the last of a (N, d) group is its tight one
PRECISION = [(5000, 128, 0), (5000, 128, 14), (5000, 128, 20), (9000, 68, 0), (9000, 68, 28), (3000, 768, 0),
             (3000, 768, 5)]
SAFE_SHARE = 0.9    # at least this share of a precision family's queries is safe
BEYOND = (5000, 128, 100)  # no query is safe: what holds when the bound does not


def gauss(N, d, offset, nq=64, seed=1):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((N, d)) + offset).astype(np.float32)
    Q = (rng.standard_normal((nq, d)) + offset).astype(np.float32)
    return X, Q


def ints(N, d, hi, nq=70, seed=1):
    assert d * hi * hi < 2 ** 22
    rng = np.random.default_rng(seed)
    X = rng.integers(0, hi + 1, (N, d)).astype(np.float32)
    Q = rng.integers(0, hi + 1, (nq, d)).astype(np.float32)
    return X, Q


def dups(N, d, nq=64, seed=1, copies=40):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d)).astype(np.float32)
    at = np.sort(rng.choice(N, copies, replace=False))
    X[at] = X[at[0]]
    Q = (X[at[0]][None, :] + 1e-3 * rng.standard_normal((nq, d))).astype(np.float32)
    return X, Q


def late(N, d, nq=32, seed=1, best=6):
    rng = np.random.default_rng(seed)
    X = np.ones((N, d), dtype=np.float32)
    X[rng.choice(np.arange(40, N), best, replace=False)] = 0.0
    Q = rng.integers(0, 2, (nq, d)).astype(np.float32)
    Q[0], Q[1] = 0.0, 1.0
    return X, Q


def true_scores(X, Q):
    """s(x) = |x|^2 - 2 x.q in float64 from the f32 inputs, [nq, N]"""
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    return (X64 * X64).sum(axis=1)[None, :] - 2.0 * (Q64 @ X64.T)


def error_bound(X, Q):
    """E_q of the docstring, [nq]"""
    X64, Q64 = np.abs(X.astype(np.float64)), np.abs(Q.astype(np.float64))
    mag = (X64 * X64).sum(axis=1)[None, :] + 2.0 * (Q64 @ X64.T)
    return 1.01 * (X.shape[1] + 2) * 2.0 ** -24 * mag.max(axis=1)


def safe(X, Q, k, oracle_ids):
    """bool per query: the screen's k + 8 must contain the oracle's top k (module docstring)"""
    S, E = true_scores(X, Q), error_bound(X, Q)
    out = np.zeros(Q.shape[0], dtype=bool)
    for qi in range(Q.shape[0]):
        ids = oracle_ids[qi][oracle_ids[qi] != PAD].astype(np.int64)
        # the count grows with s(x): the worst of the oracle's k decides
        out[qi] = ids.size == 0 or np.count_nonzero(S[qi] <= S[qi, ids].max() + 2.0 * E[qi]) <= k + SCREEN
    return out


def margin(X, Q, k, oracle_ids):
    """per query (gap between the oracle's worst kept score and the (k + 9)-th smallest score) / (2 E_q): the factor by
    which the error bound could grow before the query stops being safe; > 1 is safe (needs N > k + 8)"""
    S, E = true_scores(X, Q), error_bound(X, Q)
    nxt = np.partition(S, k + SCREEN, axis=1)[:, k + SCREEN]
    worst = np.array([S[qi, oracle_ids[qi].astype(np.int64)].max() for qi in range(Q.shape[0])])
    return (nxt - worst) / (2.0 * E)


def truncate(A, mantissa_bits):
    """f32 values with the mantissa cut (toward zero) to `mantissa_bits` explicit bits"""
    mask = np.uint32((0xFFFFFFFF << (23 - mantissa_bits)) & 0xFFFFFFFF)
    return (np.ascontiguousarray(A, dtype=np.float32).view(np.uint32) & mask).view(np.float32)


def screen_emulated(X, Q, k, mantissa_bits):
    """ids [nq, min(N, k + 8)]: the best by (score, id), the dot products from operands of `mantissa_bits` mantissa
    bits, the norms from the full f32 rows"""
    Xt, Qt = truncate(X, mantissa_bits).astype(np.float64), truncate(Q, mantissa_bits).astype(np.float64)
    X64 = X.astype(np.float64)
    S = (X64 * X64).sum(axis=1)[None, :] - 2.0 * (Qt @ Xt.T)
    keep = min(X.shape[0], k + SCREEN)
    ids = np.arange(X.shape[0])
    return np.stack([np.lexsort((ids, S[qi]))[:keep] for qi in range(Q.shape[0])]).astype(np.uint32)


def lost(screen_ids, oracle_ids):
    """bool per query: one of the oracle's ids is missing from the screen"""
    return np.array([not set(o[o != PAD].tolist()) <= set(s.tolist()) for s, o in zip(screen_ids, oracle_ids)])
