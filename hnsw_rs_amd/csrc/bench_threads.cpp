// bench_threads.cpp -- the three harness helpers that drive the public entry points from host threads of their own
// (what concurrent callers of the C ABI see, without an interpreter in the loop)

#include <sys/resource.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "handle.h"

using hx::check_search_args;
using hx::ensure_uploaded;
using hx::set_error;

extern "C" {

// T host threads, each blocked in its own hnsw_search call like the reference's callers (ann_by_vector(&self), one
// query per call): thread t answers queries t, t + T, t + 2T, ... of Q, again and again until `seconds` have passed
// and every query has been answered at least once.  ids receives each query's LAST answer (so the caller can hold
// the run to the oracle), lat_us = {p50, p90, p99, max, mean} of the per-call latencies.
int hnsw_bench_search_threads(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef, uint32_t threads,
                              double seconds, uint32_t *ids, uint32_t *counts, uint64_t *calls_out, double *wall_s,
                              double *lat_us) {
    if (!h || !Q || !ids || nq == 0 || n == 0 || threads == 0 || threads > 4096) return HNSW_ERR_ARG;
    int rc = check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    if ((rc = ensure_uploaded(h))) return rc;
    const uint32_t d = h->dev.view.dim;
    const uint32_t T = (uint32_t)std::min<uint64_t>(threads, nq);
    std::vector<std::vector<float>> lat(T);
    std::atomic<int> first_rc{HNSW_OK};
    std::string first_msg;
    std::mutex msg_mu;
    std::atomic<uint32_t> ready{0};
    std::atomic<bool> go{false};
    using clk = std::chrono::steady_clock;
    clk::time_point t_start;
    auto work = [&](uint32_t t) {
        std::vector<float> &L = lat[t];
        L.reserve(1 << 16);
        ready.fetch_add(1);
        while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
        const auto deadline = t_start + std::chrono::duration_cast<clk::duration>(std::chrono::duration<double>(seconds));
        bool full_pass = false;
        while (first_rc.load(std::memory_order_relaxed) == HNSW_OK) {
            for (uint64_t i = t; i < nq; i += T) {
                uint32_t cnt = 0;
                const auto a = clk::now();
                const int r = hnsw_search(h, Q + i * d, n, ef, ids + i * n, &cnt);
                const auto b = clk::now();
                if (counts) counts[i] = cnt;
                if (r != HNSW_OK) {
                    std::lock_guard<std::mutex> g(msg_mu);
                    if (first_rc.load() == HNSW_OK) {
                        first_msg = hx::get_error();
                        first_rc.store(r);
                    }
                    return;
                }
                L.push_back(std::chrono::duration<float, std::micro>(b - a).count());
                if (full_pass && b >= deadline) return;
            }
            full_pass = true;
            if (clk::now() >= deadline) return;
        }
    };
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < T; t++) th.emplace_back(work, t);
    while (ready.load() < T) std::this_thread::yield();
    struct rusage ru0;
    getrusage(RUSAGE_SELF, &ru0);
    t_start = clk::now();
    go.store(true, std::memory_order_release);
    for (auto &t : th) t.join();
    const double wall = std::chrono::duration<double>(clk::now() - t_start).count();
    if (first_rc.load() != HNSW_OK) {
        set_error("%s", first_msg.c_str());
        return first_rc.load();
    }
    std::vector<float> all;
    for (auto &L : lat) all.insert(all.end(), L.begin(), L.end());
    std::sort(all.begin(), all.end());
    if (calls_out) *calls_out = all.size();
    if (wall_s) *wall_s = wall;
    if (lat_us) {
        struct rusage ru1;
        getrusage(RUSAGE_SELF, &ru1);
        lat_us[5] = (ru1.ru_utime.tv_sec - ru0.ru_utime.tv_sec) + 1e-6 * (ru1.ru_utime.tv_usec - ru0.ru_utime.tv_usec);
        lat_us[6] = (ru1.ru_stime.tv_sec - ru0.ru_stime.tv_sec) + 1e-6 * (ru1.ru_stime.tv_usec - ru0.ru_stime.tv_usec);
    }
    if (lat_us && !all.empty()) {
        auto pct = [&](double p) { return (double)all[std::min(all.size() - 1, (size_t)(p * all.size()))]; };
        double sum = 0;
        for (float x : all) sum += x;
        lat_us[0] = pct(0.50);
        lat_us[1] = pct(0.90);
        lat_us[2] = pct(0.99);
        lat_us[3] = all.back();
        lat_us[4] = sum / all.size();
    }
    return HNSW_OK;
}
// The same around hnsw_search_filtered: thread t answers queries t, t + T, ... of Q, query i under row[i] of `set` (row
// NULL: no set) and the label range [lo[i], hi[i]], until `seconds` have passed and every query has been answered once.
// ids, dists (or NULL), counts, paths (or NULL) and rcs (or NULL) receive each query's LAST answer.  A per-query error
// does not end the run: it is the query's own (rcs[i]; without rcs the first one is the run's).
int hnsw_bench_search_filtered_threads(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef, hnsw_mask_set *set,
                                       const uint32_t *row, const uint32_t *lo, const uint32_t *hi, uint32_t threads,
                                       double seconds, uint32_t *ids, float *dists, uint32_t *counts, uint8_t *paths,
                                       int32_t *rcs, uint64_t *calls_out, double *wall_s, double *lat_us) {
    if (!h || !Q || !ids || !lo || !hi || nq == 0 || n == 0 || threads == 0 || threads > 4096 || (set != nullptr) != (row != nullptr))
        return HNSW_ERR_ARG;
    int rc = check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    if ((rc = ensure_uploaded(h))) return rc;
    const uint32_t d = h->dev.view.dim;
    const uint32_t T = (uint32_t)std::min<uint64_t>(threads, nq);
    std::vector<std::vector<float>> lat(T);
    std::atomic<int> first_rc{HNSW_OK};
    std::string first_msg;
    std::mutex msg_mu;
    std::atomic<uint32_t> ready{0};
    std::atomic<bool> go{false};
    using clk = std::chrono::steady_clock;
    clk::time_point t_start;
    auto work = [&](uint32_t t) {
        std::vector<float> &L = lat[t];
        L.reserve(1 << 16);
        ready.fetch_add(1);
        while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
        const auto deadline = t_start + std::chrono::duration_cast<clk::duration>(std::chrono::duration<double>(seconds));
        bool full_pass = false;
        while (first_rc.load(std::memory_order_relaxed) == HNSW_OK) {
            for (uint64_t i = t; i < nq; i += T) {
                uint32_t cnt = 0;
                uint8_t path = 0;
                const auto a = clk::now();
                const int r = hnsw_search_filtered(h, Q + i * d, n, ef, set, row ? row[i] : HNSW_MASK_NONE, lo[i], hi[i], ids + i * n,
                                                   dists ? dists + i * n : nullptr, &cnt, &path);
                const auto b = clk::now();
                if (counts) counts[i] = cnt;
                if (paths) paths[i] = path;
                if (rcs) rcs[i] = r;
                // a failure of the query alone is its answer when the caller collects them; any other ends the run
                const bool own = rcs && (r == HNSW_ERR_NAN_INPUT || r == HNSW_ERR_OVERFLOW);
                if (r != HNSW_OK && !own) {
                    std::lock_guard<std::mutex> g(msg_mu);
                    if (first_rc.load() == HNSW_OK) {
                        first_msg = hx::get_error();
                        first_rc.store(r);
                    }
                    return;
                }
                L.push_back(std::chrono::duration<float, std::micro>(b - a).count());
                if (full_pass && b >= deadline) return;
            }
            full_pass = true;
            if (clk::now() >= deadline) return;
        }
    };
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < T; t++) th.emplace_back(work, t);
    while (ready.load() < T) std::this_thread::yield();
    struct rusage ru0;
    getrusage(RUSAGE_SELF, &ru0);
    t_start = clk::now();
    go.store(true, std::memory_order_release);
    for (auto &t : th) t.join();
    const double wall = std::chrono::duration<double>(clk::now() - t_start).count();
    if (first_rc.load() != HNSW_OK) {
        set_error("%s", first_msg.c_str());
        return first_rc.load();
    }
    std::vector<float> all;
    for (auto &L : lat) all.insert(all.end(), L.begin(), L.end());
    std::sort(all.begin(), all.end());
    if (calls_out) *calls_out = all.size();
    if (wall_s) *wall_s = wall;
    if (lat_us) {
        struct rusage ru1;
        getrusage(RUSAGE_SELF, &ru1);
        lat_us[5] = (ru1.ru_utime.tv_sec - ru0.ru_utime.tv_sec) + 1e-6 * (ru1.ru_utime.tv_usec - ru0.ru_utime.tv_usec);
        lat_us[6] = (ru1.ru_stime.tv_sec - ru0.ru_stime.tv_sec) + 1e-6 * (ru1.ru_stime.tv_usec - ru0.ru_stime.tv_usec);
    }
    if (lat_us && !all.empty()) {
        auto pct = [&](double p) { return (double)all[std::min(all.size() - 1, (size_t)(p * all.size()))]; };
        double sum = 0;
        for (float x : all) sum += x;
        lat_us[0] = pct(0.50);
        lat_us[1] = pct(0.90);
        lat_us[2] = pct(0.99);
        lat_us[3] = all.back();
        lat_us[4] = sum / all.size();
    }
    return HNSW_OK;
}
// `callers` host threads, each calling hnsw_search_batch (host pointers in and out) `calls` times on its own slice
// of Q (caller t takes queries [t * nq, (t + 1) * nq) modulo total) into its own result buffers: what concurrent
// batch callers of the C ABI see, without an interpreter in the loop.  *wall_s = the time from the first call to the
// last return (every caller's stream and staging exist before the clock starts: two untimed calls each).
int hnsw_bench_batch_threads(hnsw_index *h, const float *Q, uint64_t total, uint64_t nq, uint32_t n, uint32_t ef,
                             uint32_t callers, uint32_t calls, double *wall_s) {
    if (!h || !Q || !wall_s || nq == 0 || total < nq || n == 0 || callers == 0 || callers > 64 || calls == 0) return HNSW_ERR_ARG;
    int rc = check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    if ((rc = ensure_uploaded(h))) return rc;
    const uint32_t d = h->dev.view.dim;
    std::atomic<int> first_rc{HNSW_OK};
    std::string first_msg;
    std::mutex msg_mu;
    std::atomic<uint32_t> ready{0};
    std::atomic<bool> go{false};
    const uint64_t slices = total / nq;
    auto work = [&](uint32_t t) {
        std::vector<uint32_t> ids(nq * n), counts(nq);
        std::vector<float> dists(nq * n);
        std::vector<hnsw_query_stats> st(nq);
        auto one = [&](uint32_t i) {
            const float *q = Q + ((t + (uint64_t)i * callers) % slices) * nq * d;
            return hnsw_search_batch(h, q, nq, n, ef, ids.data(), dists.data(), counts.data(), st.data());
        };
        int r = one(0);
        if (r == HNSW_OK) r = one(1);
        ready.fetch_add(1);
        while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
        for (uint32_t i = 0; i < calls && r == HNSW_OK && first_rc.load(std::memory_order_relaxed) == HNSW_OK; i++) r = one(i + 2);
        if (r != HNSW_OK) {
            std::lock_guard<std::mutex> g(msg_mu);
            if (first_rc.load() == HNSW_OK) {
                first_msg = hx::get_error();
                first_rc.store(r);
            }
        }
    };
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < callers; t++) th.emplace_back(work, t);
    while (ready.load() < callers) std::this_thread::yield();
    const auto t0 = std::chrono::steady_clock::now();
    go.store(true, std::memory_order_release);
    for (auto &t : th) t.join();
    *wall_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (first_rc.load() != HNSW_OK) {
        set_error("%s", first_msg.c_str());
        return first_rc.load();
    }
    return HNSW_OK;
}

}  // extern "C"
