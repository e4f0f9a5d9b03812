// coalesce.h -- coalescing of concurrent one-query calls (hnsw_search = the shim's ann_by_vector); internal.
// A handle holds one Coalescer by value, so the types live here; the scheme itself is coalesce.cpp.
//
// The reference answers ONE query per call and takes &self, so its callers are many threads each blocked in its
// own call (template.rs:306-335).  A lone query is a lone wave: ~130 us on a machine that answers 1024 queries in
// the same time.  Concurrent calls on one handle are therefore gathered: a caller claims a slot of the open batch
// (one compare-and-swap on the batch's word: no lock on this path -- hundreds of callers taking turns on a mutex
// that each holds for 100 ns spend their time in futex hand-offs, measured: 256 callers, 15 cores of system time),
// copies its query into the batch's pinned staging area and sleeps on one of the batch's futex words; the caller
// that claimed slot 0 is the batch's LEADER: it closes the batch, launches ONE kernel for everything that arrived,
// hands every caller its ids and wakes them.  Every query of a batch is answered by its own wave exactly as a lone
// query would be, so the result of a call does not depend on what it was batched with.
//   window:  a leader that has seen concurrency (the previous batch held more than one query) waits up to
//            `window_us` for the callers that were woken together with it to come back; a lone caller never waits.
//   depth:   at most `depth` batches are on the GPU at once; leaders beyond that keep collecting arrivals.
//
// One-query FILTERED calls (hnsw_search_filtered) gather the same way, in batches of their own: a batch's parameters
// are (n, ef, dim, filtered?, set), and a caller joins only a batch whose parameters are its own.  A filtered slot
// stages the caller's (row, lo, hi) next to its query; the leader states the batch's filter once -- the rows of `set`
// (or every id), one label range per query, the staged arrays -- and answers it by search_filtered with the exact path
// in its grouped form: the queries on the graph path share one launch whatever their filters, those on the exact path
// three (filter_exact.cpp, exact_grouped).  With the window off (coalesce_us < 0) a filtered call still comes through
// here, as a batch of its own that nobody else sees.
#pragma once

#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "scratch.h"

struct hnsw_index;
struct hnsw_mask_set;

namespace hx {

struct SpinLock {  // the slow paths' lock: a short spin, then sleep on the word (free / held / held with sleepers)
    std::atomic<uint32_t> v{0};
    void lock() {
        for (int spins = 0; spins < 128; spins++) {
            uint32_t exp = 0;
            if (v.load(std::memory_order_relaxed) == 0 && v.compare_exchange_weak(exp, 1, std::memory_order_acquire)) return;
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
        }
        while (v.exchange(2, std::memory_order_acquire) != 0)
            (void)syscall(SYS_futex, reinterpret_cast<uint32_t *>(&v), FUTEX_WAIT_PRIVATE, 2, nullptr, nullptr, 0);
    }
    void unlock() {
        if (v.exchange(0, std::memory_order_release) == 2)
            (void)syscall(SYS_futex, reinterpret_cast<uint32_t *>(&v), FUTEX_WAKE_PRIVATE, 1, nullptr, nullptr, 0);
    }
};

struct CoBatch {
    SearchScratch s;
    size_t p_q = 0, p_out = 0;  // pinned arena offsets (HostSearchPlan for `cap` queries)
    size_t p_row = 0, p_lo = 0, p_hi = 0;  // a filtered batch: [queries | rows | lo | hi | result block]
    // (n, ef, dim, cap, filtered, set) of this incarnation; written before the word's generation is bumped, read by joiners
    std::atomic<uint32_t> cap{0}, n{0}, ef{0}, dim{0}, filtered{0};
    std::atomic<void *> set{nullptr};
    // bits 0..15: slots claimed; bit 16: closed (no more joins); bits 32..63: generation (a batch is reused).
    // A joiner's compare-and-swap succeeds only on the word it read its parameters under.
    static constexpr uint64_t COUNT = 0xFFFFull, CLOSED = 1ull << 16, GEN = 1ull << 32;
    // a batch of COUNT slots is full (cobatch_join), so a joiner's + 1 never carries into CLOSED: the option
    // "coalesce_max" is held to COUNT
    static_assert(COUNT + 1 == CLOSED && CLOSED < GEN, "the slot count sits right below the closed bit");
    std::atomic<uint64_t> word{CLOSED};
    std::atomic<uint32_t> filed{0};  // claimed slots whose query and request are in place
    struct Req {
        uint32_t *ids, *count;
        float *dists;   // a filtered call's (or nullptr)
        uint8_t *path;
    };
    std::vector<Req> reqs;
    // futex words, 0 = collecting / running, 1 = results handed out; callers spread over them by slot
    struct alignas(64) Word {
        std::atomic<uint32_t> v{0};
    };
    static constexpr uint32_t WORDS = 16;
    Word done[WORDS];
    std::atomic<uint32_t> readers{0};  // followers that have not picked up their status yet
    int rc = HNSW_OK;                  // batch-level failure (launch, copy), with its text
    std::string err;
    std::vector<int32_t> status;       // per query
    std::vector<uint8_t> paths;        // per query of a filtered batch
};
struct Coalescer {
    std::atomic<CoBatch *> fast{nullptr};  // the open batch callers try first (the latest parameters seen)
    SpinLock mu;                           // everything below; callers on the fast path never take it
    std::condition_variable_any cv;        // leaders wait here for a place on the GPU
    std::vector<CoBatch *> open;           // every open batch, `fast` included
    std::vector<std::unique_ptr<CoBatch>> all;
    std::vector<CoBatch *> idle;
    uint32_t in_flight = 0;
    std::atomic<uint32_t> last_size{1};
    // options "coalesce_us" (< 0: off, every call launches by itself), "coalesce_depth", "coalesce_max"
    std::atomic<int64_t> window_us{30};
    uint32_t depth = 3, cap = 1024;
    std::atomic<uint64_t> n_batches{0}, n_queries{0}, max_batch{0};
    // where a leader's time goes, in ns (hnsw_get_stat "coalesce_ns_window" / "_turn" / "_gpu" / "_handout")
    std::atomic<uint64_t> ns_window{0}, ns_turn{0}, ns_gpu{0}, ns_handout{0};
    // under mu: the open batches nobody has joined (a leaderless successor made for other parameters or another
    // device) are closed and go back to the pool; `fast` is cleared if it was one of them
    void retire_unjoined();
    CoBatch *take();  // under mu: a batch from the pool, or a new one
};

// hnsw_search through the coalescer (the arguments are checked by the caller)
int search_coalesced(hnsw_index *h, const float *q, uint32_t n, uint32_t ef, uint32_t *ids, uint32_t *count);
// hnsw_search_filtered through it: under row `row` of `set` (nullptr: no rows; HNSW_MASK_NONE: no row) AND the label range
// [lo, hi].  alone: the call gathers nobody and waits for nobody (coalesce_us < 0, or parameters whose errors depend on
// what else is in the batch)
int search_filtered_coalesced(hnsw_index *h, const float *q, uint32_t n, uint32_t ef, hnsw_mask_set *set, uint32_t row,
                              uint32_t lo, uint32_t hi, uint32_t *ids, float *dists, uint32_t *count, uint8_t *path, bool alone);

}  // namespace hx
