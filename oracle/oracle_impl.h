// oracle_impl.h -- the CPU oracle's internals, shared by oracle.cpp and batched_build.cpp.
//
// TEST INFRASTRUCTURE, NOT PRODUCT CODE (see oracle.h).  Not part of the C interface: the types
// and functions that restate the reference (graph, points, Searcher, Inserter, HNSW::insert), so
// that a second restatement can be built from them instead of from copies.
// All citations are relative to /root/reference/.
#ifndef HNSW_ORACLE_IMPL_H
#define HNSW_ORACLE_IMPL_H

#include "oracle.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <set>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace orc {

typedef uint32_t NodeID;  // graph/src/lib.rs:1

// vectors crate (oracle.cpp): QuantVec::distance_unrolled, FullVec::distance
float dist_quant(uint32_t d, const uint8_t *cx, float delta_x, float min_x, const uint8_t *cy,
                 float delta_y, float min_y);
float dist_full(uint32_t d, const float *x, const float *y);


// ---------------------------------------------------------------------------------------------
// graph crate
// ---------------------------------------------------------------------------------------------

// graph/src/dist.rs:4-38
struct Dist {
    NodeID id;
    float dist;
};
inline int dist_cmp(const Dist &a, const Dist &b) {
    if (a.dist < b.dist) return -1;
    if (a.dist > b.dist) return 1;
    if (a.dist == b.dist) return a.id < b.id ? -1 : (a.id > b.id ? 1 : 0);
    return -2;  // NaN: partial_cmp().unwrap() panics
}
struct DistLess {
    bool operator()(const Dist &a, const Dist &b) const { return dist_cmp(a, b) == -1; }
};
typedef std::set<Dist, DistLess> OrderedDists;  // BTreeSet<Dist>

// IntSet<NodeID> as a sorted vector with set semantics (iteration = ascending id)
struct IdSet {
    std::vector<NodeID> v;
    bool insert(NodeID x) {
        auto it = std::lower_bound(v.begin(), v.end(), x);
        if (it != v.end() && *it == x) return false;
        v.insert(it, x);
        return true;
    }
    bool remove(NodeID x) {
        auto it = std::lower_bound(v.begin(), v.end(), x);
        if (it == v.end() || *it != x) return false;
        v.erase(it);
        return true;
    }
    size_t len() const { return v.size(); }
};

enum GraphErr { G_OK = 0, G_NODE_NOT_IN_GRAPH, G_SELF_CONNECTION };

// graph/src/graph.rs:9-16
struct Graph {
    std::unordered_map<NodeID, IdSet> nodes;
    size_t level;
    size_t m;

    // graph.rs:31-35
    void add_node(NodeID id) { nodes.emplace(id, IdSet()); }
    // graph.rs:37-52
    GraphErr add_edge(NodeID a, NodeID b, NodeID *bad = nullptr) {
        if (a == b) {
            if (bad) *bad = a;
            return G_SELF_CONNECTION;
        }
        auto ia = nodes.find(a), ib = nodes.find(b);
        if (ia == nodes.end() || ib == nodes.end()) {  // graph.rs:54-70
            if (bad) *bad = (ia != nodes.end()) ? b : a;
            return G_NODE_NOT_IN_GRAPH;
        }
        ia->second.insert(b);
        ib->second.insert(a);
        return G_OK;
    }
    // graph.rs:72-83
    GraphErr remove_edge(NodeID a, NodeID b) {
        auto ia = nodes.find(a), ib = nodes.find(b);
        if (ia == nodes.end() || ib == nodes.end()) return G_NODE_NOT_IN_GRAPH;
        ia->second.remove(b);
        ib->second.remove(a);
        return G_OK;
    }
    // graph.rs:150-155
    bool degree(NodeID n, size_t *out) const {
        auto it = nodes.find(n);
        if (it == nodes.end()) return false;
        *out = it->second.len();
        return true;
    }
    // graph.rs:103-113
    bool neighbors_vec(NodeID n, std::vector<NodeID> *out) const {
        auto it = nodes.find(n);
        if (it == nodes.end()) return false;
        *out = it->second.v;
        return true;
    }
    // graph.rs:85-94
    GraphErr isolate_node(NodeID node) {
        std::vector<NodeID> nb;
        if (!neighbors_vec(node, &nb)) return G_NODE_NOT_IN_GRAPH;
        for (NodeID neighbor : nb) {
            size_t deg;
            if (!degree(neighbor, &deg)) return G_NODE_NOT_IN_GRAPH;
            if (deg == 1) continue;
            GraphErr e = remove_edge(node, neighbor);
            if (e != G_OK) return e;
        }
        return G_OK;
    }
    // graph.rs:140-148
    template <class It>
    GraphErr add_neighbors(NodeID node, It begin, It end) {
        for (It it = begin; it != end; ++it) {
            GraphErr e = add_edge(node, *it);
            if (e != G_OK) return e;
        }
        return G_OK;
    }
    // graph.rs:128-138
    template <class It>
    GraphErr replace_neighbors(NodeID node, It begin, It end) {
        GraphErr e = isolate_node(node);
        if (e != G_OK) return e;
        return add_neighbors(node, begin, end);
    }
    // iter_nodes (graph.rs:27-29) in this oracle's documented order: ascending id
    std::vector<NodeID> iter_nodes() const {
        std::vector<NodeID> ids;
        ids.reserve(nodes.size());
        for (auto &kv : nodes) ids.push_back(kv.first);
        std::sort(ids.begin(), ids.end());
        return ids;
    }
};

// graph/src/layers.rs:7-70
struct Layers {
    std::vector<Graph> levels;
    size_t m;
    size_t len() const { return levels.size(); }
    void add_level(size_t level) {  // layers.rs:48-59
        while (len() <= level) {
            Graph g;
            g.level = len();
            g.m = (len() == 0) ? m * 2 : m;
            levels.push_back(std::move(g));
        }
    }
    void add_node(NodeID id, size_t level) {  // layers.rs:63-70
        add_level(level);
        for (size_t l = 0; l <= level && l < levels.size(); l++) levels[l].add_node(id);
    }
};

// ---------------------------------------------------------------------------------------------
// points crate (SimplePoints as SoA; arithmetic unchanged)
// ---------------------------------------------------------------------------------------------

struct PointRef {  // points/src/point.rs:6-10 (a view)
    NodeID id = 0;
    uint8_t level = 0;
    const uint8_t *codes = nullptr;
    float delta = 0.0f, min = 0.0f;
    const float *vals = nullptr;
};

struct Points {
    int kind;
    uint32_t dim;
    std::vector<uint8_t> codes;
    std::vector<float> mins, deltas;
    std::vector<float> vals;
    std::vector<uint8_t> levels;
    size_t len() const { return levels.size(); }
    bool get_point(NodeID idx, PointRef *p) const {  // points.rs:75-77
        if ((size_t)idx >= len()) return false;
        p->id = idx;
        p->level = levels[idx];
        if (kind == ORC_VEC_QUANT8) {
            p->codes = &codes[(size_t)idx * dim];
            p->delta = deltas[idx];
            p->min = mins[idx];
            p->vals = nullptr;
        } else {
            p->codes = nullptr;
            p->delta = p->min = 0.0f;
            p->vals = &vals[(size_t)idx * dim];
        }
        return true;
    }
};

// Point::dist2other -> VecType::dist2other (points/src/point.rs:35-37)
inline float dist2other(const Points &pts, const PointRef &a, const PointRef &b) {
    if (pts.kind == ORC_VEC_QUANT8)
        return dist_quant(pts.dim, a.codes, a.delta, a.min, b.codes, b.delta, b.min);
    return dist_full(pts.dim, a.vals, b.vals);
}

// ---------------------------------------------------------------------------------------------
// hnsw crate
// ---------------------------------------------------------------------------------------------

// hnsw/src/params.rs:5-42
struct Params {
    NodeID ep;
    size_t m, mmax, mmax0;
    float ml;
    size_t ef_cons, dim;
};

typedef std::map<NodeID, OrderedDists> LayerResult;    // IntMap<NodeID, OrderedDists>
typedef std::map<size_t, LayerResult> LayersResults;   // IntMap<usize, LayerResult>

struct Counters {
    uint64_t n_dist = 0, n_exp = 0, sum_deg = 0;
};

// hnsw/src/template/results.rs:26-45
struct Results {
    OrderedDists selected, candidates;
    std::unordered_set<NodeID> visited;
    OrderedDists visited_h;
    LayersResults insertion_results, prune_results;
    void clear_all() {  // results.rs:182-190
        selected.clear();
        candidates.clear();
        visited.clear();
        visited_h.clear();
        insertion_results.clear();
        prune_results.clear();
    }
};

}  // namespace orc

struct orc_index {
    orc::Params params;
    orc::Layers layers;
    orc::Points points;
};

namespace orc {

typedef orc_index HNSW;

// hnsw/src/template/searcher.rs:23-103  Searcher::search_layer
int search_layer(Results &results, const Graph &layer, const PointRef &point, const HNSW &index,
                 size_t ef, Counters *ctr);
// what one select_heuristic call did: candidates before any cap, candidates popped
struct HeuristicTrace {
    size_t n_cands = 0, n_popped = 0;
};
// searcher.rs:109-153 select_heuristic; cand_cap > 0 keeps only the cand_cap nearest candidates
int select_heuristic(Results &results, const Graph &layer, const PointRef &point,
                     const Points &points, size_t m, bool extend_cands, bool keep_pruned,
                     size_t cand_cap = 0, HeuristicTrace *trace = nullptr);
// template.rs:614-621 select_simple
OrderedDists select_simple(std::vector<Dist> cands, size_t m);

// hnsw/src/template/inserter.rs:19-127
struct Inserter {
    Results results;

    int build_insertion_results(const HNSW &index, const PointRef &point) {
        if (point.id == index.params.ep) return ORC_OK;  // inserter.rs:42-45 (results left stale)
        // setup_insert, inserter.rs:53-68
        results.clear_all();
        PointRef ep;
        if (!index.points.get_point(index.params.ep, &ep)) return ORC_ERR_ARG;
        const float dist2ep = dist2other(index.points, ep, point);  // index.distance(ep, point.id)
        if (std::isnan(dist2ep)) return ORC_ERR_NAN;
        results.selected.insert(Dist{index.params.ep, dist2ep});
        // traverse_layers_above, inserter.rs:70-89
        const size_t layers_len = index.layers.len();
        for (size_t layer_nb = layers_len; layer_nb-- > (size_t)point.level + 1;) {
            int rc = search_layer(results, index.layers.levels[layer_nb], point, index, 1, nullptr);
            if (rc != ORC_OK) return rc;
        }
        // traverse_layers_below, inserter.rs:91-126
        const size_t bound = std::min((size_t)point.level, layers_len - 1);
        for (size_t layer_nb = bound + 1; layer_nb-- > 0;) {
            const Graph &layer = index.layers.levels[layer_nb];
            int rc = search_layer(results, layer, point, index, index.params.ef_cons, nullptr);
            if (rc != ORC_OK) return rc;
            rc = select_heuristic(results, layer, point, index.points, index.params.m, true, true);
            if (rc != ORC_OK) return rc;
            // results.rs:79-84 save_layer_results
            results.insertion_results[layer_nb][point.id] = results.selected;
        }
        return ORC_OK;
    }
};

// template.rs:177-190 insert (+196-251)
int insert(HNSW &index, NodeID point_id, Inserter &inserter);
// template.rs:269-293 store_points: stores the rows, adds the nodes to their layers, sets the ep
int store_points(HNSW &index, const float *rows, uint64_t n, const uint8_t *levels,
                 std::vector<NodeID> *ids_out);

}  // namespace orc

#endif
