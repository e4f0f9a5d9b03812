// batched_build.cpp -- CPU restatement of the product's batch-synchronous on-device build
// (option "gpu_build" = 2, hnsw_insert_bulk_device, and what every rank of the sharded build
// computes).  TEST INFRASTRUCTURE, NOT PRODUCT CODE (see oracle.h): it includes and links nothing
// of hnsw_rs_amd/, and is built from the oracle's own search_layer, select_heuristic, insert,
// Graph and dist2other (oracle_impl.h).  The device build is deterministic for a given batch
// schedule, so tests/test_gpu_build_restatement.py requires its graph to equal this one edge for
// edge.  The rules, one step each ("Order and batching"):
//
//  1. Order.   Levels top-down, ids ascending within a level, the entry point excluded.
//  2. Seed.    The first min(|order|, 2048 - n_before) points (none once the index holds 2048)
//              are inserted by the oracle's sequential insert -- the reference's algorithm, with
//              its candidate leak and transient over-cap rows.  If that
//              is every point, or the index has more than 16 layers (edge records carry 4-bit
//              layers), every point is inserted that way and nothing below applies.
//  3. Clamp.   Layers ascending, nodes ascending: a row longer than its layer's cap (2 m on
//              layer 0, m above) is pruned as the reference's next prune_connections would --
//              select_simple keeps the cap nearest by (dist, id), the dropped edges are removed on
//              both sides -- unless a dropped edge is that neighbour's only one: then the neighbour
//              keeps it, and the clamped side gets it back after the build (rule 8).  This runs
//              whenever a batch follows, also when there was no seed.
//  4. Batches. The next batch takes min(rest, min(BMAX, batch_max), max(64, connected /
//              batch_div)) points of the order, BMAX = 32768; `connected` starts at n_before plus
//              the seed and grows by each batch.
//  5. Phase 1. Every point of a batch is searched against the graph as it stood at the batch's
//              start: setup from the entry point, greedy descent with ef = 1 above its level,
//              then on each layer <= min(level, top layer): search_layer(ef_cons),
//              select_heuristic(m, extend, keep_pruned).  Two deviations from the reference: the
//              heuristic's candidate set (selected + their neighbours) is cut to its 512 nearest
//              by (dist, id) before the first pop, and the un-popped candidates do not leak into
//              the next layer's search.  The point's own row on a layer is its selection.
//              Points of a batch are independent: they run on `nthreads` threads, which changes
//              nothing in the result.
//  6. Phase 2. Every selected neighbour n of a batch point p is a request (layer, n <- p) with
//              d(p, n).  Each target row takes its requests in ascending source id: if
//              row + sources fit the cap, the sources are appended; otherwise the row keeps the
//              cap nearest of existing + sources by (dist, id) -- dist2other for the existing
//              neighbours -- and every one that falls out, source or not, is a removal
//              (layer, x -> n).
//  7. Phase 3. After every row of phase 2: each x drops, in ascending id, the neighbours that
//              dropped it and are still in its row -- except when that neighbour is the row's
//              only one: the edge stays and the refusal (layer, x, n) is recorded.
//  8. Mirror.  After the final batch, for every refusal and clamp restore (layer, x, n): if x
//              still holds n and n does not hold x, n gets x back (the product's read_graph).
//
// Points the product sends to its CPU path (insert-kernel status other than a visited-table
// overflow, or an overflow again with the larger table) are not modelled: the tests require that
// there are none.
// All citations are relative to /root/reference/.

#include <thread>

#include "oracle_impl.h"

namespace orc {
namespace {

constexpr size_t SEED = 2048, BMAX = 32768, CAND_CAP = 512, WINDOW = 128, MAX_BATCHED_LAYERS = 16;

// how often phase 1's heuristic went where the kernel's special paths are: a candidate set cut to
// CAND_CAP, more than WINDOW candidates popped (the kernel's sweep window grows past its first 128)
struct Reach {
    uint64_t cut = 0, past_window = 0;
};

struct Edge {  // (layer, row, other) with d(row, other)
    uint32_t layer;
    NodeID row, other;
    float dist;
};
inline bool edge_less(const Edge &a, const Edge &b) {
    if (a.layer != b.layer) return a.layer < b.layer;
    if (a.row != b.row) return a.row < b.row;
    return a.other < b.other;
}
inline bool same_row(const Edge &a, const Edge &b) { return a.layer == b.layer && a.row == b.row; }

inline bool holds(const IdSet &s, NodeID x) { return std::binary_search(s.v.begin(), s.v.end(), x); }

// rule 1
std::vector<NodeID> insertion_order(const HNSW &index, const std::vector<NodeID> &ids) {
    std::vector<NodeID> order;
    for (int l = 255; l >= 0; l--)
        for (NodeID id : ids)  // ids ascending (store_points)
            if (id != index.params.ep && index.points.levels[id] == (uint8_t)l) order.push_back(id);
    return order;
}

// rule 3: the prune the reference would make next (prune_connections / select_simple,
// template.rs:209-238,614-621, remove_edge / isolate_node, graph.rs:72-94) -- except that an edge
// which is the dropped neighbour's only one leaves the clamped row until rule 8 puts it back
void clamp_rows(HNSW &index, std::vector<Edge> *restore) {
    for (uint32_t l = 0; l < index.layers.len(); l++) {
        Graph &g = index.layers.levels[l];
        for (NodeID id : g.iter_nodes()) {
            std::vector<NodeID> nbrs;
            g.neighbors_vec(id, &nbrs);
            if (nbrs.size() <= g.m) continue;
            PointRef a, b;
            index.points.get_point(id, &a);
            std::vector<Dist> ds;
            for (NodeID x : nbrs) {
                index.points.get_point(x, &b);
                ds.push_back(Dist{x, dist2other(index.points, a, b)});
            }
            IdSet keep;
            for (const Dist &k : select_simple(ds, g.m)) keep.insert(k.id);
            for (NodeID x : nbrs) {
                if (holds(keep, x)) continue;
                size_t deg = 0;
                g.degree(x, &deg);
                if (deg == 1) {  // x's only edge: x keeps it, id gets it back after the build
                    g.nodes[id].remove(x);
                    restore->push_back(Edge{l, x, id, 0.0f});
                } else {
                    g.remove_edge(id, x);
                }
            }
        }
    }
}

// rule 5: the selections of point p on layers 0 .. min(level, top), against the graph as it is
// ((*sel)[l] for those layers only: the point is on no other)
int batch_search(const HNSW &index, NodeID p, std::vector<std::vector<Dist>> *sel, Reach *reach) {
    PointRef point, ep;
    if (!index.points.get_point(p, &point) || !index.points.get_point(index.params.ep, &ep))
        return ORC_ERR_ARG;
    Results results;
    const float d_ep = dist2other(index.points, ep, point);
    if (std::isnan(d_ep)) return ORC_ERR_NAN;
    results.selected.insert(Dist{index.params.ep, d_ep});
    const size_t layers_len = index.layers.len();
    for (size_t l = layers_len; l-- > (size_t)point.level + 1;) {
        int rc = search_layer(results, index.layers.levels[l], point, index, 1, nullptr);
        if (rc != ORC_OK) return rc;
    }
    const size_t bound = std::min((size_t)point.level, layers_len - 1);
    sel->assign(bound + 1, {});
    for (size_t l = bound + 1; l-- > 0;) {
        const Graph &layer = index.layers.levels[l];
        results.candidates.clear();  // no leak of the heuristic's un-popped candidates
        int rc = search_layer(results, layer, point, index, index.params.ef_cons, nullptr);
        if (rc != ORC_OK) return rc;
        HeuristicTrace tr;
        rc = select_heuristic(results, layer, point, index.points, index.params.m, true, true, CAND_CAP, &tr);
        if (rc != ORC_OK) return rc;
        reach->cut += tr.n_cands > CAND_CAP;
        reach->past_window += tr.n_popped > WINDOW;
        (*sel)[l].assign(results.selected.begin(), results.selected.end());
    }
    return ORC_OK;
}

// rules 5-7 for one batch; refusals of phase 3 are appended to *refusals
int run_batch(HNSW &index, const NodeID *batch, size_t B, int nthreads, std::vector<Edge> *refusals, Reach *reach) {
    // ---- phase 1 ----
    std::vector<std::vector<std::vector<Dist>>> sel(B);
    std::vector<int> rcs(nthreads, ORC_OK);
    std::vector<Reach> reach_t(nthreads);
    auto work = [&](int t) {
        for (size_t i = B * t / nthreads; i < B * (t + 1) / nthreads; i++) {
            const int rc = batch_search(index, batch[i], &sel[i], &reach_t[t]);
            if (rc != ORC_OK) rcs[t] = rc;
        }
    };
    if (nthreads == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < nthreads; t++) th.emplace_back(work, t);
        for (auto &x : th) x.join();
    }
    for (int rc : rcs)
        if (rc != ORC_OK) return rc;
    for (const Reach &r : reach_t) {
        reach->cut += r.cut;
        reach->past_window += r.past_window;
    }
    std::vector<Edge> req;
    for (size_t i = 0; i < B; i++) {
        for (uint32_t l = 0; l < sel[i].size(); l++) {
            IdSet &own = index.layers.levels[l].nodes[batch[i]];
            for (const Dist &n : sel[i][l]) {
                own.insert(n.id);
                req.push_back(Edge{l, n.id, batch[i], n.dist});
            }
        }
    }
    // ---- phase 2 ----
    std::sort(req.begin(), req.end(), edge_less);
    std::vector<Edge> rem;
    for (size_t lo = 0, hi; lo < req.size(); lo = hi) {
        for (hi = lo + 1; hi < req.size() && same_row(req[hi], req[lo]);) hi++;
        Graph &g = index.layers.levels[req[lo].layer];
        const NodeID n = req[lo].row;
        IdSet &row = g.nodes[n];
        if (row.len() + (hi - lo) <= g.m) {
            for (size_t j = lo; j < hi; j++) row.insert(req[j].other);
            continue;
        }
        PointRef a, b;
        index.points.get_point(n, &a);
        std::vector<Dist> ds;
        for (NodeID x : row.v) {
            index.points.get_point(x, &b);
            ds.push_back(Dist{x, dist2other(index.points, a, b)});
        }
        for (size_t j = lo; j < hi; j++) ds.push_back(Dist{req[j].other, req[j].dist});
        std::sort(ds.begin(), ds.end(), DistLess());
        row.v.clear();
        for (size_t i = 0; i < ds.size(); i++) {
            if (i < g.m)
                row.insert(ds[i].id);
            else
                rem.push_back(Edge{req[lo].layer, ds[i].id, n, 0.0f});
        }
    }
    // ---- phase 3 ----
    std::sort(rem.begin(), rem.end(), edge_less);
    for (const Edge &e : rem) {
        IdSet &row = index.layers.levels[e.layer].nodes[e.row];
        if (!holds(row, e.other)) continue;
        if (row.len() == 1)
            refusals->push_back(e);
        else
            row.remove(e.other);
    }
    return ORC_OK;
}

}  // namespace
}  // namespace orc

using namespace orc;

extern "C" int orc_insert_bulk_batched(orc_index *h, const float *rows, uint64_t n, const uint8_t *levels,
                                       uint32_t batch_max, uint32_t batch_div, int nthreads, uint64_t *stats) {
    if (batch_max == 0 || batch_div == 0 || h->params.m > 128 || h->params.ef_cons > 512) return ORC_ERR_ARG;
    if (nthreads < 1) nthreads = 1;
    HNSW &index = *h;
    const uint64_t n_before = index.points.len();
    std::vector<NodeID> ids;
    int rc = store_points(index, rows, n, levels, &ids);
    if (rc != ORC_OK) return rc;
    const std::vector<NodeID> order = insertion_order(index, ids);
    // ---- rule 2 ----
    const size_t take = n_before < SEED ? std::min<size_t>(order.size(), SEED - n_before) : 0;
    const bool sequential = take == order.size() || index.layers.len() > MAX_BATCHED_LAYERS;
    Inserter inserter;
    for (size_t i = 0; i < (sequential ? order.size() : take); i++)
        if ((rc = insert(index, order[i], inserter)) != ORC_OK) return rc;
    uint64_t n_batches = 0;
    Reach reach;
    std::vector<Edge> restore, refusals;
    if (!sequential) {
        clamp_rows(index, &restore);  // rule 3
        uint64_t connected = n_before + take;
        for (size_t pos = take; pos < order.size();) {  // rule 4
            const size_t B = std::min<size_t>(
                order.size() - pos,
                std::min<uint64_t>(std::min<uint64_t>(BMAX, batch_max), std::max<uint64_t>(64, connected / batch_div)));
            if ((rc = run_batch(index, &order[pos], B, nthreads, &refusals, &reach)) != ORC_OK) return rc;
            pos += B;
            connected += B;
            n_batches++;
        }
    }
    // ---- rule 8 ----
    const size_t n_refusals = refusals.size();
    refusals.insert(refusals.end(), restore.begin(), restore.end());
    for (const Edge &e : refusals) {
        Graph &g = index.layers.levels[e.layer];
        if (holds(g.nodes[e.row], e.other) && !holds(g.nodes[e.other], e.row)) g.nodes[e.other].insert(e.row);
    }
    if (stats) {
        stats[0] = sequential ? order.size() : take;  // points inserted sequentially
        stats[1] = n_batches;
        stats[2] = n_refusals + restore.size();  // kept-last-edges: phase 3 refusals + clamp restores
        stats[3] = restore.size();
        stats[4] = reach.cut;
        stats[5] = reach.past_window;
    }
    return ORC_OK;
}
