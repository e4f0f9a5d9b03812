"""What the tests of search from stored rows share (tests/test_from_rows_host.py, tests/test_gpu_from_rows.py): a second,
deliberately plain statement of the fold and of the drop -- scalar loops over one element and one entry at a time, no
numpy operation on more than a scalar -- and the synthetic slots and lists of the sweeps.  A helper of the tests, no tests
of its own and no pytest."""
import itertools

import numpy as np

MAX = 0xFFFFFFFF
OK, ERR_NAN_INPUT, ERR_ARG = 0, -2, -8

WIDTHS = (1, 2, 3, 64)
N_INS = (1, 63, 64, 65, 200, 1024)
DROP_WIDTHS = (1, 3, 64)
NQ = 12  # queries of a synthetic drop case


def n_outs(n_in):
    return sorted({1, min(10, n_in), n_in})


# ---- the plain statements -----------------------------------------------------------------------------------------------
def naive_compose(src_ids, weights, get_row, n_points, dim):
    """the contract's fold, one scalar at a time -> rows [nq, dim], statuses [nq]"""
    src_ids = np.asarray(src_ids, dtype=np.uint32)
    nq, width = src_ids.shape
    rows = np.zeros((nq, dim), dtype=np.float32)
    statuses = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        present = [s for s in range(width) if int(src_ids[q, s]) != MAX]
        if len(present) == 0 or any(int(src_ids[q, s]) >= n_points for s in present):
            statuses[q] = ERR_ARG
            continue
        stored = {s: np.asarray(get_row(int(src_ids[q, s])), dtype=np.float32) for s in present}
        with np.errstate(invalid="ignore", over="ignore"):
            for e in range(dim):
                acc = None
                for s in present:
                    w = np.float32(1.0) if weights is None else np.float32(weights[q][s])
                    p = np.float32(w * np.float32(stored[s][e]))
                    acc = p if acc is None else np.float32(acc + p)
                rows[q, e] = acc
    return rows, statuses


def naive_drop(ids, dists, counts, statuses, ex, n_out, src_statuses=None):
    """the contract's drop, one entry at a time -> ids, dists, counts, dropped, statuses"""
    ids, dists, ex = np.asarray(ids, dtype=np.uint32), np.asarray(dists, dtype=np.float32), np.asarray(ex, dtype=np.uint32)
    nq, n_in = ids.shape
    o_ids = np.full((nq, n_out), MAX, dtype=np.uint32)
    o_dists = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_counts, dropped = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
    out_status = np.zeros(nq, dtype=np.int64) if statuses is None else np.array(statuses, dtype=np.int64)
    for q in range(nq):
        ok = out_status[q] == OK
        if src_statuses is not None and int(src_statuses[q]) != OK:
            out_status[q] = int(src_statuses[q])
            ok = False
        if not ok:
            continue
        listed = [int(x) for x in ex[q] if int(x) != MAX]
        w = 0
        for j in range(n_in):
            present = j < min(int(counts[q]), n_in) if counts is not None else int(ids[q, j]) != MAX
            if not present:
                continue
            if int(ids[q, j]) in listed:
                dropped[q] += 1
                continue
            if w < n_out:
                o_ids[q, w], o_dists[q, w] = ids[q, j], dists[q, j]
            w += 1
        o_counts[q] = min(w, n_out)
    return o_ids, o_dists, o_counts, dropped, out_status


def assert_drop_equal(got, want, what=""):
    """ids, distance BITS, counts (and dropped, where both sides have it) equal"""
    assert np.array_equal(np.asarray(got[2]), np.asarray(want[2])), "%s: counts differ: %s vs %s" % (what, got[2], want[2])
    assert np.array_equal(got[0], want[0]), "%s: ids differ" % what
    assert np.array_equal(np.asarray(got[1]).view(np.uint32), np.asarray(want[1]).view(np.uint32)), "%s: distance bits differ" % what
    if len(got) > 3 and got[3] is not None and want[3] is not None:
        assert np.array_equal(np.asarray(got[3]), np.asarray(want[3])), "%s: dropped differs: %s vs %s" % (what, got[3], want[3])


# ---- synthetic slots of the compose sweep --------------------------------------------------------------------------------
def compose_slots(width, n_points, seed, nq=16):
    """src_ids [nq, width] below n_points with pads at the front (query 1), in the middle (2), at the end (3), a query of
    pads only (4), an id equal to the length (5), one slot alone present (6), a repeated id (7); weights with negative,
    zero, +inf (query 8) and NaN (query 9) members"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n_points, (nq, width)).astype(np.uint32)
    w = (rng.random((nq, width), dtype=np.float32) * np.float32(4) - np.float32(2)).astype(np.float32)
    w[:, ::3] = np.abs(w[:, ::3])
    w[0, 0] = 0.0
    w[10, :] = -w[10, :]
    if width > 1:
        src[1, 0] = MAX
        src[2, width // 2] = MAX
        src[3, width - 1] = MAX
        src[7, :] = src[7, 0]
        if width > 2:
            src[11, ::2] = MAX  # every other slot
    src[6, :] = MAX
    src[6, width - 1] = 11 % n_points
    src[4, :] = MAX
    src[5, width - 1] = n_points
    w[8, width - 1] = np.inf
    w[9, 0] = np.nan
    return src, w


# ---- synthetic lists of the drop sweep -----------------------------------------------------------------------------------
def drop_lists(n_in, width, with_counts, seed, id_span=1500):
    """[NQ][n_in] candidate lists and [NQ][width] exclusion lists:
      query 0  the excluded id sits first          1  in the middle          2  last          3  nowhere (absent)
      4  an id twice in the list, excluded         5  an exclusion id given twice (where width allows)
      6  a failed incoming status                  7  every present entry excluded (where width allows; else one)
      8  pads in the exclusion list against pads in the entries (without counts: pads in the middle of the list)
      9  count 0 (with counts) / a list of pads only          10  a count above n_in / a full list
      11  a failed compose status (src_statuses)
    -> ids, dists, counts or None, statuses, ex, src_statuses"""
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.permutation(id_span)[:n_in] for _ in range(NQ)]).astype(np.uint32)  # (n_in <= id_span)
    dists = np.sort(rng.random((NQ, n_in), dtype=np.float32), axis=1)
    counts = rng.integers(max(1, n_in // 2), n_in + 1, NQ).astype(np.uint32)
    ex = np.full((NQ, width), MAX, dtype=np.uint32)
    far = np.uint32(id_span + 7)  # an id no list holds
    ex[:, 0] = far
    last = lambda q: (int(counts[q]) if with_counts else n_in) - 1  # noqa: E731
    ex[0, 0] = ids[0, 0]
    ex[1, 0] = ids[1, last(1) // 2]
    ex[2, width - 1] = ids[2, last(2)]
    if n_in >= 3:
        ids[4, last(4)] = ids[4, 0]
    ex[4, 0] = ids[4, 0]
    if width >= 2:
        ex[5, 0] = ex[5, 1] = ids[5, 0]
        if width >= 3:
            ex[5, 2] = ids[5, last(5)]
    k = min(width, n_in)
    ex[7, :k] = ids[7, :k]
    if with_counts:
        counts[7] = k
    else:
        ids[7, k:] = MAX
    ex[8, :] = MAX
    if width >= 2:
        ex[8, 1] = ids[8, 0]
    if not with_counts and n_in >= 3:
        ids[8, 1:n_in:3] = MAX
    counts[9] = 0
    if not with_counts:
        ids[9, :] = MAX
    counts[10] = n_in + 5
    ex[10, 0] = ids[10, n_in - 1]
    statuses = np.zeros(NQ, dtype=np.int64)
    statuses[6] = ERR_NAN_INPUT
    src_statuses = np.zeros(NQ, dtype=np.int32)
    src_statuses[11] = ERR_ARG
    ex[11, 0] = ids[11, 0]
    return ids, dists, (counts if with_counts else None), statuses, ex, src_statuses


def drop_sweep():
    return list(itertools.product(N_INS, DROP_WIDTHS))
