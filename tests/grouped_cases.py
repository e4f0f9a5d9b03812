"""What the grouped-search tests share (tests/test_grouped_host.py, tests/test_gpu_grouped.py): a deliberately naive
restatement of THE COLLAPSE of include/hnsw_mi355x.h ("grouped search") -- a dict and a loop per query, nothing in common
with hnsw_rs_amd.grouped.group_by_label's array code -- and the synthetic candidate lists both are swept over."""
import numpy as np

MAX = 0xFFFFFFFF
POOLS = (1, 63, 64, 65, 128, 255, 256)
NQ = 24
N_LABELS = 600  # the label column the synthetic lists are made for


def shapes(pool):
    """(n_groups, per_group) of the sweep at a pool: per_group in {1, 2, pool} x n_groups in {1, 3, pool}, those within
    the limits (both <= pool, product <= 1024)"""
    out = []
    for P in (1, 2, pool):
        for G in (1, 3, pool):
            if G <= pool and P <= pool and G * P <= 1024 and (G, P) not in out:
                out.append((G, P))
    return out


def column():
    """the labels of ids 0 .. N_LABELS - 1: ids 0..255 all distinct (and large), ids 256..511 all 77, the rest from
    {0, 1, 2, 3, UINT32_MAX}"""
    lab = np.zeros(N_LABELS, dtype=np.uint32)
    lab[:256] = 100000 + 3 * np.arange(256)
    lab[256:512] = 77
    lab[512:] = np.random.default_rng(9).choice(np.array([0, 1, 2, 3, MAX], dtype=np.uint32), N_LABELS - 512)
    return lab


def synthetic_lists(pool, with_counts, seed):
    """NQ candidate lists of `pool` entries over column()'s ids and ids beyond it (label 0), distinct within a list as a
    search returns them.  query 0: nothing present;  1: every label the same;  2: every label distinct;  3: labels 0 and
    UINT32_MAX and 1..3 only;  4: ids beyond the column only (one group, label 0);  5: full;  the rest ragged.  With
    counts, the entries beyond a count hold live-looking ids that must not be read as present (and query 6's count is
    above pool: clamped); without, they are pads -- and pads stand in the MIDDLE of the lists of queries 7.. as well."""
    rng = np.random.default_rng(seed)
    ids = np.zeros((NQ, pool), dtype=np.uint32)
    dists = np.sort(rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 3.0], dtype=np.float32), (NQ, pool)), axis=1)
    counts = np.zeros(NQ, dtype=np.uint32)
    for q in range(NQ):
        if q == 1:
            row = 256 + rng.permutation(256)[:pool]
        elif q == 2:
            row = rng.permutation(256)[:pool]
        elif q == 3:
            row = 512 + rng.permutation(max(pool, N_LABELS - 512 + 40))[:pool]  # (ids from N_LABELS on: label 0)
        elif q == 4:
            row = N_LABELS + rng.permutation(1000)[:pool]
        else:
            row = rng.permutation(N_LABELS + 150)[:pool]
        c = pool if q in (1, 2, 3, 4, 5) else int(rng.integers(0, pool + 1))
        if q == 0:
            c = 0
        ids[q], counts[q] = row, c
        if not with_counts:
            ids[q, c:], dists[q, c:] = MAX, np.inf
            if q >= 7 and c > 2:
                holes = rng.choice(c, max(1, c // 5), replace=False)
                ids[q, holes], dists[q, holes] = MAX, np.inf
    if with_counts:
        counts[6] = pool + 5
    return ids, dists, (counts if with_counts else None)


def naive(ids, dists, counts, labels, n_groups, per_group):
    """THE COLLAPSE, one query and one entry at a time"""
    nq, pool = ids.shape
    G, P = n_groups, per_group
    o_ids = np.full((nq, G, P), MAX, dtype=np.uint32)
    o_bits = np.full((nq, G, P), 0x7F800000, dtype=np.uint32)
    o_labels = np.zeros((nq, G), dtype=np.uint32)
    o_sizes = np.zeros((nq, G), dtype=np.uint32)
    o_counts = np.zeros(nq, dtype=np.uint32)
    bits = np.ascontiguousarray(dists, dtype=np.float32).view(np.uint32)
    for q in range(nq):
        number, members = {}, {}  # label -> the group's number; label -> entries seen
        for j in range(pool):
            if counts is not None:
                if j >= min(int(counts[q]), pool):
                    continue
            elif int(ids[q, j]) == MAX:
                continue
            i = int(ids[q, j])
            label = int(labels[i]) if labels is not None and i < len(labels) else 0
            if label not in number:
                number[label] = len(number)
                members[label] = 0
            g, r = number[label], members[label]
            members[label] += 1
            if g < G and r < P:
                o_ids[q, g, r] = i
                o_bits[q, g, r] = bits[q, j]
        for label, g in number.items():
            if g < G:
                o_labels[q, g] = label
                o_sizes[q, g] = min(P, members[label])
        o_counts[q] = min(G, len(number))
    return o_ids, o_bits.view(np.float32), o_labels, o_sizes, o_counts


def assert_grouped_equal(got, want, what):
    """ids, distance BITS, group labels, sizes and counts"""
    assert np.array_equal(np.asarray(got[4]).astype(np.uint32), want[4]), what + ": counts"
    assert np.array_equal(got[0], want[0]), what + ": ids"
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.uint32), np.ascontiguousarray(want[1]).view(np.uint32)), \
        what + ": distance bits"
    assert np.array_equal(got[2], want[2]), what + ": group labels"
    assert np.array_equal(got[3], want[3]), what + ": group sizes"
