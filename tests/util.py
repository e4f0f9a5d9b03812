"""Shared helpers of the parity tests."""
import numpy as np

import hnsw_rs_amd as H
from oracle import oracle_py as O


def oracle_from_product(index, vectors, levels):
    """An oracle index holding exactly the product index's points and graph (the oracle quantises
    the same float rows itself, so identical codes are part of what is being checked)."""
    orc = O.OracleHNSW(int(index.params.m), int(index.params.ef_cons), index.dim, index.vec_kind)
    orc.import_points(vectors, levels)
    for l in range(index.nb_layers()):
        ids, offs, nbrs = index.get_layer(l).csr()
        orc.import_layer(l, ids, offs, nbrs)
    orc.set_ep(int(index.params.ep))
    return orc


def product_from_oracle(orc, vectors, levels):
    idx = H.HNSW.new(orc.m, None, orc.dim, orc.vec_kind)
    idx.import_points(vectors, levels)
    for l in range(orc.nb_layers):
        ids, offs, nbrs = orc.layer_csr(l)
        idx.import_layer(l, ids, offs, nbrs)
    idx.set_ep(orc.ep)
    return idx


def same_graph(index, orc):
    if index.nb_layers() != orc.nb_layers or int(index.params.ep) != orc.ep:
        return False
    for l in range(orc.nb_layers):
        a, b = index.get_layer(l).csr(), orc.layer_csr(l)
        if not all(np.array_equal(x, y) for x, y in zip(a, b)):
            return False
    return True


def graph_difference(idx, orc):
    """None if the product index and the oracle index hold the same graph, else a message naming the first differing
    (layer, node), its missing and extra neighbours and their dist2other to the node (near-tie or real error?)"""
    if int(idx.params.ep) != orc.ep:
        return "entry point %d, restatement %d" % (int(idx.params.ep), orc.ep)
    if idx.nb_layers() != orc.nb_layers:
        return "%d layers, restatement %d" % (idx.nb_layers(), orc.nb_layers)
    for l in range(orc.nb_layers):
        ids, offs, nbrs = idx.get_layer(l).csr()
        o_ids, o_offs, o_nbrs = orc.layer_csr(l)
        if not np.array_equal(ids, o_ids):
            return "layer %d: node ids differ (%d vs %d nodes)" % (l, len(ids), len(o_ids))
        if np.array_equal(offs, o_offs) and np.array_equal(nbrs, o_nbrs):
            continue
        for k, node in enumerate(ids.tolist()):
            got = set(nbrs[int(offs[k]):int(offs[k + 1])].tolist())
            want = set(o_nbrs[int(o_offs[k]):int(o_offs[k + 1])].tolist())
            if got == want:
                continue
            fmt = lambda xs: ", ".join("%d (d=%r)" % (x, float(orc.distance(node, x))) for x in sorted(xs))
            n_rows = sum(1 for j in range(len(ids)) if not np.array_equal(
                np.asarray(nbrs[int(offs[j]):int(offs[j + 1])]), np.asarray(o_nbrs[int(o_offs[j]):int(o_offs[j + 1])])))
            return ("layer %d, node %d (of %d differing rows on the layer): missing [%s], extra [%s]; the row's "
                    "largest kept distance in the restatement %r" %
                    (l, node, n_rows, fmt(want - got), fmt(got - want),
                     max((float(orc.distance(node, x)) for x in want), default=None)))
    return None


def rand_vectors(n, d, seed):
    """make_rand_vectors (hnsw/src/template.rs:630-638): U[0,1)"""
    return np.random.Generator(np.random.PCG64(seed)).random((n, d), dtype=np.float32)


def assert_search_equal(got, want, what=""):
    """ids bit-exact, distances bit-exact (0 ulp; the stated tolerance is 1e-4), counters equal"""
    g_ids, g_d, g_c, g_s = got
    w_ids, w_d, w_c, w_s = want
    assert np.array_equal(g_c, w_c), what + " counts differ"
    bad = np.nonzero((g_ids != w_ids).any(axis=1))[0]
    assert bad.size == 0, "%s ids differ for queries %s: got %s want %s" % (
        what, bad[:5], g_ids[bad[:2]], w_ids[bad[:2]])
    mask = w_ids != O.UINT32_MAX
    assert np.array_equal(g_d[mask].view(np.uint32), w_d[mask].view(np.uint32)), what + " distances differ"
    assert np.allclose(g_d[mask], w_d[mask], rtol=0, atol=1e-4)
    assert np.array_equal(np.asarray(g_s)[:, :3], np.asarray(w_s)[:, :3].astype(np.int64)), \
        what + " counters (n_dist, n_exp, sum_deg) differ"
