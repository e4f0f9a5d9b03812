// coalesce.cpp -- hnsw_search through the coalescer: concurrent one-query calls on a handle are gathered into one
// launch (coalesce.h explains the scheme)

#include "coalesce.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <mutex>
#include <thread>

#include "handle.h"
#include "search_host.h"

namespace hx {

namespace {

inline void futex_wait(std::atomic<uint32_t> *w, uint32_t while_equals) {
    while (w->load(std::memory_order_acquire) == while_equals)
        (void)syscall(SYS_futex, reinterpret_cast<uint32_t *>(w), FUTEX_WAIT_PRIVATE, while_equals, nullptr, nullptr, 0);
}
// Waking n sleepers from one thread costs that thread n wake-ups one after the other (a hundred microseconds for
// a hundred callers): the leader wakes two, and every caller that wakes up wakes two more.  The word is already 1
// by then, so a caller that was not asleep yet never goes to sleep and no wake-up can be lost.
inline void futex_wake(std::atomic<uint32_t> *w, int n) {
    (void)syscall(SYS_futex, reinterpret_cast<uint32_t *>(w), FUTEX_WAKE_PRIVATE, n, nullptr, nullptr, 0);
}

// a batch from the pool made ready for a new incarnation with `claimed` slots already taken (1: the caller leads
// it; 0: a leaderless successor whose first joiner will); called under Coalescer::mu
// what a batch is opened and joined by, and what a caller brings
struct CoCall {
    const float *q;
    uint32_t n, ef;
    uint32_t *ids, *count;
    bool filtered = false;
    hnsw_mask_set *set = nullptr;
    uint32_t row = HNSW_MASK_NONE, lo = 0, hi = 0xFFFFFFFFu;
    float *dists = nullptr;
    uint8_t *path = nullptr;
    bool alone = false;
};

int cobatch_open(hnsw_index *h, CoBatch &b, uint32_t cap, const CoCall &c, uint32_t claimed) {
    const uint32_t d = h->dev.view.dim, n = c.n, ef = c.ef;
    int rc;
    if (c.filtered) {
        // the device arena is search_filtered's own lease; pinned: [queries | rows | lo | hi | result block]
        b.p_q = 0;
        b.p_row = align256((size_t)cap * d * 4);
        b.p_lo = b.p_row + align256((size_t)cap * 4);
        b.p_hi = b.p_lo + align256((size_t)cap * 4);
        b.p_out = b.p_hi + align256((size_t)cap * 4);
        if ((rc = b.s.reserve(h->dev.device, 0, b.p_out + ResultBlock(cap, n).bytes, false)) != HNSW_OK) return rc;
        if (b.paths.size() < cap) b.paths.resize(cap);
    } else {
        const HostSearchPlan p = plan_host_search(cap, d, n, 0);
        if ((rc = b.s.reserve(h->dev.device, p.dev_bytes, p.pin_bytes, false)) != HNSW_OK) return rc;  // (exactly what the plan asks for)
        b.p_q = p.p_q;
        b.p_out = p.p_out;
    }
    b.cap.store(cap, std::memory_order_relaxed);
    b.n.store(n, std::memory_order_relaxed);
    b.ef.store(ef, std::memory_order_relaxed);
    b.dim.store(d, std::memory_order_relaxed);
    b.filtered.store(c.filtered ? 1 : 0, std::memory_order_relaxed);
    b.set.store(c.set, std::memory_order_relaxed);
    b.filed.store(0, std::memory_order_relaxed);
    for (auto &w : b.done) w.v.store(0, std::memory_order_relaxed);
    b.readers.store(0, std::memory_order_relaxed);
    b.rc = HNSW_OK;
    b.err.clear();
    if (b.reqs.size() < cap) b.reqs.resize(cap);
    if (b.status.size() < cap) b.status.resize(cap);
    const uint64_t gen = (b.word.load(std::memory_order_relaxed) >> 32) + 1;
    b.word.store((gen << 32) | claimed, std::memory_order_release);  // open
    return HNSW_OK;
}

// claim a slot of an open batch with these parameters: the slot, or -1 (closed, full, other parameters)
inline int cobatch_join(CoBatch *b, const CoCall &c, uint32_t d) {
    const uint32_t n = c.n, ef = c.ef;
    uint64_t w = b->word.load(std::memory_order_acquire);
    while (true) {
        if ((w & CoBatch::CLOSED) || (w & CoBatch::COUNT) >= b->cap.load(std::memory_order_relaxed)) return -1;
        if (b->n.load(std::memory_order_relaxed) != n || b->ef.load(std::memory_order_relaxed) != ef ||
            b->dim.load(std::memory_order_relaxed) != d || b->filtered.load(std::memory_order_relaxed) != (c.filtered ? 1u : 0u) ||
            b->set.load(std::memory_order_relaxed) != (void *)c.set)
            return -1;
        // succeeds only if the word is still the one the parameters were read under (same generation, still open)
        if (b->word.compare_exchange_weak(w, w + 1, std::memory_order_acq_rel, std::memory_order_acquire))
            return (int)(w & CoBatch::COUNT);
    }
}

// the snapshot is what the host index holds (read without the handle's lock: nothing may mutate an index while
// it is being searched, include/hnsw_mi355x.h)
inline bool snapshot_current(const hnsw_index *h) {
    return h->dev.valid && (h->dev.replica || h->dev.version_seen == h->host->version);
}

}  // namespace

CoBatch *Coalescer::take() {
    if (idle.empty()) {
        all.emplace_back(new CoBatch());
        return all.back().get();
    }
    CoBatch *b = idle.back();
    idle.pop_back();
    return b;
}

void Coalescer::retire_unjoined() {
    for (size_t i = 0; i < open.size();) {
        CoBatch *o = open[i];
        uint64_t w = o->word.load(std::memory_order_acquire);
        if ((w & CoBatch::COUNT) == 0 && !(w & CoBatch::CLOSED) &&
            o->word.compare_exchange_strong(w, w | CoBatch::CLOSED, std::memory_order_acq_rel)) {
            open.erase(open.begin() + i);
            idle.push_back(o);
            if (fast.load(std::memory_order_relaxed) == o) fast.store(nullptr, std::memory_order_release);
        } else {
            i++;
        }
    }
}

namespace {

int coalesced(hnsw_index *h, const CoCall &c) {
    const float *q = c.q;
    const uint32_t n = c.n, ef = c.ef;
    uint32_t *ids = c.ids, *count = c.count;
    int rc;
    if (!snapshot_current(h) && (rc = ensure_uploaded(h)) != HNSW_OK) return rc;
    Coalescer &co = h->co;
    const uint32_t d = h->dev.view.dim;
    // ---- claim a slot: the open batch everybody looks at first, else (under the lock) any open batch with these
    // parameters, else a new batch which this caller leads ----
    CoBatch *b = c.alone ? nullptr : co.fast.load(std::memory_order_acquire);
    int slot = b ? cobatch_join(b, c, d) : -1;
    if (slot < 0 && c.alone) {
        // a batch of its own, open to nobody: slot 0 of one, never listed
        std::lock_guard<SpinLock> g(co.mu);
        b = co.take();
        if ((rc = cobatch_open(h, *b, 1, c, 1)) != HNSW_OK) {
            co.idle.push_back(b);
            return rc;
        }
        slot = 0;
    } else if (slot < 0) {
        std::lock_guard<SpinLock> g(co.mu);
        for (CoBatch *o : co.open)
            if ((slot = cobatch_join(o, c, d)) >= 0) {
                b = o;
                break;
            }
        if (slot < 0) {
            // a leaderless batch nobody joined (other parameters) is taken out of circulation rather than left open
            co.retire_unjoined();
            b = co.take();
            if ((rc = cobatch_open(h, *b, co.cap, c, 1)) != HNSW_OK) {
                co.idle.push_back(b);
                return rc;
            }
            slot = 0;
            co.open.push_back(b);
            co.fast.store(b, std::memory_order_release);
        }
    }
    unsigned char *const pin = static_cast<unsigned char *>(b->s.pin);
    memcpy(pin + b->p_q + (size_t)slot * d * 4, q, (size_t)d * 4);
    if (c.filtered) {
        reinterpret_cast<uint32_t *>(pin + b->p_row)[slot] = c.row;
        reinterpret_cast<uint32_t *>(pin + b->p_lo)[slot] = c.lo;
        reinterpret_cast<uint32_t *>(pin + b->p_hi)[slot] = c.hi;
    }
    b->reqs[slot] = CoBatch::Req{ids, count, c.dists, c.path};
    b->filed.fetch_add(1, std::memory_order_release);

    if (slot != 0) {
        std::atomic<uint32_t> *word = &b->done[slot % CoBatch::WORDS].v;
        futex_wait(word, 0);
        futex_wake(word, 2);
        int my = b->rc;
        if (my != HNSW_OK)
            set_error("%s", b->err.c_str());
        else
            my = query_status_error(0, b->status[slot]);
        if (b->readers.fetch_sub(1, std::memory_order_acq_rel) == 1) {  // the last one out returns the batch
            std::lock_guard<SpinLock> g(co.mu);
            co.idle.push_back(b);
        }
        return my;
    }

    // ---- leader (slot 0) ----
    using sclk = std::chrono::steady_clock;
    auto ns_since = [](sclk::time_point t) { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(sclk::now() - t).count(); };
    const auto t_lead = sclk::now();
    const int64_t window_us = co.window_us.load(std::memory_order_relaxed);
    const uint32_t last = co.last_size.load(std::memory_order_relaxed);
    if (window_us > 0 && last > 1 && !c.alone) {
        // callers woken together come back together: wait for as many as the previous batch held, at most the
        // window (spinning: a timed sleep of tens of microseconds wakes up 50 us late)
        const uint32_t target = std::min(last, b->cap.load(std::memory_order_relaxed));
        const auto deadline = t_lead + std::chrono::microseconds(window_us);
        while ((b->word.load(std::memory_order_acquire) & CoBatch::COUNT) < target && sclk::now() < deadline) {
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
        }
    }
    co.ns_window.fetch_add(ns_since(t_lead), std::memory_order_relaxed);
    const auto t_turn = sclk::now();
    if (!c.alone) {
        std::unique_lock<SpinLock> lk(co.mu);
        while (co.in_flight >= co.depth) co.cv.wait(lk);
        co.in_flight++;
        co.open.erase(std::find(co.open.begin(), co.open.end(), b));
        if (co.fast.load(std::memory_order_relaxed) == b) {
            // the successor is published BEFORE this batch closes, so that arrivals always find an open batch without
            // the lock; it has no leader yet: whoever claims its slot 0 will be
            CoBatch *nx = co.take();
            if (cobatch_open(h, *nx, co.cap, c, 0) == HNSW_OK) {
                co.open.push_back(nx);
                co.fast.store(nx, std::memory_order_release);
            } else {
                co.idle.push_back(nx);
                co.fast.store(nullptr, std::memory_order_release);
            }
        }
    }
    co.ns_turn.fetch_add(ns_since(t_turn), std::memory_order_relaxed);
    const uint32_t nq = (uint32_t)(b->word.fetch_or(CoBatch::CLOSED, std::memory_order_acq_rel) & CoBatch::COUNT);
    for (uint32_t spins = 0; b->filed.load(std::memory_order_acquire) != nq; spins++) {
        // joiners between their claim and their copy (~100 ns) -- unless one of them was descheduled right there
        // (a throttled CPU quota can hold a thread for a whole period): then stop burning the core it needs
        if (spins < 2000) {
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
        } else {
            std::this_thread::yield();
        }
    }
    if (!c.alone) co.last_size.store(nq, std::memory_order_relaxed);
    if (!c.filtered) {  // (a filtered batch counts under filtered_one_calls / _batches, when it has been answered)
        co.n_batches.fetch_add(1, std::memory_order_relaxed);
        co.n_queries.fetch_add(nq, std::memory_order_relaxed);
        uint64_t mb = co.max_batch.load(std::memory_order_relaxed);
        while (nq > mb && !co.max_batch.compare_exchange_weak(mb, nq)) {
        }
    }
    HostSearchPlan p = plan_host_search(nq, d, n, 0);  // the device arena and the result block are laid out for nq
    p.p_q = b->p_q;
    p.p_out = b->p_out;  // (the pinned result block starts where the batch's capacity put it)
    DevView dummy{};
    dummy.nb_layers = h->dev.view.nb_layers;
    SearchArgs a = ann_args(dummy, nullptr, n, ef, nullptr, nullptr, nullptr, nullptr);
    const auto t_gpu = sclk::now();
    rc = hipSetDevice(h->dev.device) == hipSuccess ? HNSW_OK : HNSW_ERR_HIP;
    if (rc != HNSW_OK) set_error("hipSetDevice(%d) failed", h->dev.device);
    if (rc == HNSW_OK && c.filtered) {
        // the batch's filter, stated once: the rows of the callers' set (or every id) and a label range per query, the
        // staged arrays; the exact path of its groups in the grouped form
        Filter f;
        f.family = Filter::ONE_QUERY;
        f.rows = c.set ? Filter::SET : Filter::ALL;
        f.set = c.set;
        f.mask_of = c.set ? reinterpret_cast<const uint32_t *>(pin + b->p_row) : nullptr;
        f.K = 1;
        f.lo = reinterpret_cast<const uint32_t *>(pin + b->p_lo);
        f.hi = reinterpret_cast<const uint32_t *>(pin + b->p_hi);
        rc = search_filtered(h, reinterpret_cast<const float *>(pin + p.p_q), nq, n, ef, f, false, nullptr, nullptr, nullptr,
                             nullptr, b->paths.data(), pin + p.p_out, true);
    } else if (rc == HNSW_OK && h->del.count) {
        // ids are deleted: the batch is answered as hnsw_search_batch answers it then, into the same result block
        rc = search_filtered(h, reinterpret_cast<const float *>(pin + p.p_q), nq, n, ef, Filter{}, false, nullptr, nullptr,
                             nullptr, nullptr, nullptr, pin + p.p_out);
    } else if (rc == HNSW_OK) {
        rc = search_staged(h, b->s, p, a, nq, nullptr, nullptr);
    }
    co.ns_gpu.fetch_add(ns_since(t_gpu), std::memory_order_relaxed);
    const auto t_hand = sclk::now();
    if (!c.alone) {
        {
            std::lock_guard<SpinLock> g(co.mu);
            co.in_flight--;
        }
        co.cv.notify_all();
    }
    int my;
    if (rc != HNSW_OK) {
        b->rc = rc;
        b->err = get_error();
        my = rc;
    } else {
        const ResultBlock::Ptrs o = p.out.at(static_cast<unsigned char *>(b->s.pin) + p.p_out);
        for (uint32_t i = 0; i < nq; i++) {
            memcpy(b->reqs[i].ids, o.ids + (size_t)i * n, (size_t)n * 4);
            if (b->reqs[i].count) *b->reqs[i].count = o.counts[i];
            if (b->reqs[i].dists) memcpy(b->reqs[i].dists, o.dists + (size_t)i * n, (size_t)n * 4);
            if (b->reqs[i].path) *b->reqs[i].path = b->paths[i];
            b->status[i] = o.stats[i].status;
        }
        my = query_status_error(0, b->status[0]);
    }
    if (nq > 1) {
        b->readers.store(nq - 1, std::memory_order_release);
        for (uint32_t w = 0; w < std::min(nq, CoBatch::WORDS); w++) {
            b->done[w].v.store(1, std::memory_order_release);
            futex_wake(&b->done[w].v, 2);
        }
    } else {
        std::lock_guard<SpinLock> g(co.mu);
        co.idle.push_back(b);
    }
    co.ns_handout.fetch_add(ns_since(t_hand), std::memory_order_relaxed);
    return my;
}

}  // namespace

int search_coalesced(hnsw_index *h, const float *q, uint32_t n, uint32_t ef, uint32_t *ids, uint32_t *count) {
    CoCall c{q, n, ef, ids, count};
    return coalesced(h, c);
}

int search_filtered_coalesced(hnsw_index *h, const float *q, uint32_t n, uint32_t ef, hnsw_mask_set *set, uint32_t row,
                              uint32_t lo, uint32_t hi, uint32_t *ids, float *dists, uint32_t *count, uint8_t *path, bool alone) {
    CoCall c{q, n, ef, ids, count};
    c.filtered = true;
    c.set = set, c.row = row, c.lo = lo, c.hi = hi;
    c.dists = dists, c.path = path;
    c.alone = alone;
    return coalesced(h, c);
}

}  // namespace hx
