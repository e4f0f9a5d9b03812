// pair_kernel.inc -- included by search_lean.hip (inside namespace hx { namespace { ... } }).
//
// HNSW::ann_by_vector (hnsw/src/template.rs:306-335) over FullVec rows with TWO waves per query (round 4).
// At batch 1024 the one-wave kernel above is a chain of ~ 30 k dependent instructions per query with nothing else to
// issue (profiles/latency_floor_latest.json: 8.6 k cycles per layer-0 pass, 3.4 k of them list maintenance); the L1
// path is a third used (profiles/r04_ta_tcp_counters.txt).  Here the traversal and the list are decoupled:
//
//   wave 0, the WALKER, owns the query, the visited table and the rows: upper layers, then per layer-0 pass the
//           adjacency rows of the pair (c, p), look, row gather, FullVec's chain, claims -- and it decides from the
//           keys it has just computed whether p commits and which pair comes next;
//   wave 1, the KEEPER, owns the sorted list: it merges each pass's keys, marks c and p expanded, applies the
//           termination rule (searcher.rs:35, 41-44) and publishes the list's four smallest unexpanded entries (F).
//
// The walker never waits for a merge in the steady state: it picks the next pair from F of the pass BEFORE (which the
// keeper finished long ago) and this pass's keys -- the two smallest of {F[2], F[3], c's fresh keys, p's fresh keys}
// when p commits (no fresh key of c sorts in front of p), of {F[1], F[2], c's fresh keys} when it does not -- and runs
// the next gather while the keeper merges.  Every pass is CHECKED against the keeper's F before anything it did is
// counted or sent on: F[0] must be the c it expanded (F[1] the p).  The one way a pick can be wrong is a key that fell
// off the list's end (the keeper truncates to ef), and then nothing unexpanded is left: the search is over and the
// speculative gather is dropped -- its claims went into a visited set nobody will read again.  Any other mismatch
// (none is known) gives the query up with HNSW_ERR_OVERFLOW, which the callers run again through the one-wave kernel.
// Rows with an overflow pointer (degree > S0: imported graphs only) take the same exit.
//
// Same list, same visited set, same distances, same counters as hx_lean_f32_kernel: the parity tests run both.
// Messages go through LDS (a wave's LDS operations are served in order): the writer stores data, then a sequence word;
// the reader loads the sequence word FIRST and the data behind it in the same round trip, and takes the data only when
// the word says so.  No acknowledgements: F of pass k is published after the keys of pass k - 1 were taken out of the
// box, and the walker writes the keys of pass k only after it has seen F of pass k.  Every poll is bounded and raises
// `abort` for both waves when it runs out.

#ifdef HX_PAIR_DEBUG
#define HX_PAIR_EXIT(code) (-(100 + (code)))
#else
#define HX_PAIR_EXIT(code) HNSW_ERR_OVERFLOW
#endif
struct PairBox {
    u64 keys[64];       // walker -> keeper: this pass's keys (LK_INVALID = none); lanes 0..31 c's, 32..63 p's
    // keeper -> walker: the list's smallest unexpanded entries before pass f_seq - 1 (0 of them: the search is over)
    uint32_t f_seq, f_n, pad0, pad1;
    u64 f_key[4];
    // walker -> keeper: k_seq 1 = the entry point's key, k + 2 = the keys of pass k; k_flags bit 0: p committed
    uint32_t k_seq, k_flags, b_done;
    int32_t b_status;
    uint32_t abort, pad2, pad3, pad4;
};

// The box lives in LDS and is read and written as LDS: a `volatile` access through a generic pointer compiles to a
// system-scope FLAT load with a full wait behind each one (seven of them made one poll cost ~ 1.1 k cycles); relaxed
// workgroup-scope atomics on address-space-3 pointers are plain ds_read / ds_write that the compiler neither caches
// nor reorders across the barriers below, and the LDS serves a wave's requests in order.
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) u64 lds_u64;
__device__ __forceinline__ uint32_t box_load(const uint32_t *p) {
    return __hip_atomic_load((const lds_u32 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ u64 box_load64(const u64 *p) {
    return __hip_atomic_load((const lds_u64 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void box_store(uint32_t *p, uint32_t v) {
    asm volatile("" ::: "memory");
    __hip_atomic_store((lds_u32 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ u64 uni64(u64 x) { return ((u64)uni((uint32_t)(x >> 32)) << 32) | uni((uint32_t)x); }
constexpr uint32_t PAIR_POLLS = 1u << 21;

template <int DS, class LT>
__global__ void __launch_bounds__(128) hx_pair_f32_kernel(const LeanArgs a) {
    constexpr int R = LT::NR;
    static_assert(DS % 4 == 0, "whole 16-byte pieces");
    static_assert(R <= 2, "one register, or head + tail: entry 64 r + lane");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const uint32_t role = uni(threadIdx.x >> 6);  // 0 walker, 1 keeper
    const uint32_t q = a.qsel ? a.qsel[blockIdx.x] : blockIdx.x;
    const uint32_t hslots = 1u << a.slots_log2;
    u64 *perm = reinterpret_cast<u64 *>(smem + 4ull * hslots);
    PairBox *box = reinterpret_cast<PairBox *>(smem + 4ull * hslots + (64ull * R + 64) * 8);
    const uint32_t ef = max(1u, a.ef);

    if (threadIdx.x < 4) (&box->f_seq)[threadIdx.x] = 0;
    if (threadIdx.x >= 64 && threadIdx.x < 72) (&box->k_seq)[threadIdx.x - 64] = 0;
    __syncthreads();

    if (role == 1) {
        // ============================== the keeper ==============================
        __builtin_amdgcn_s_setprio(0);  // (it has slack: where it shares a SIMD with a walker, the walker issues first)
        LT lst;
        lst.init();
        int32_t status = HNSW_OK;
        PP_STATE();
        bool is_p[2] = {false, false};  // this lane's entry (of register r) is the pass's runner-up
        for (uint32_t k = 0;; k++) {  // message k: 0 = the entry point's key, k >= 1 = the keys of pass k - 1
            [[maybe_unused]] const unsigned long long w0 = PP_NOW();
            uint32_t seq = 0, flags = 0;
            u64 key = LK_INVALID;
            bool got = false;
            for (uint32_t it = 0; it < PAIR_POLLS; it++) {  // (the word alone: four keepers poll on every CU)
                seq = box_load(&box->k_seq);
                const uint32_t ab = box_load(&box->abort);
                if (uni(seq) >= k + 1u) {
                    got = true;
                    break;
                }
                if (uni(ab) != 0) break;
                __builtin_amdgcn_s_sleep(1);
            }
            asm volatile("" ::: "memory");
            flags = box_load(&box->k_flags);
            key = box_load64(&box->keys[lane]);
            if (!got) {
                box_store(&box->abort, 1u);
                break;
            }
            PP_ADD(PAIR_K_WAIT_KEYS, w0);
            [[maybe_unused]] const unsigned long long m0 = PP_NOW();
            flags = uni(flags);
            [[maybe_unused]] const bool upper = lane >= 32;
            if (k == 0) {
                lst.set_first(uni64(key), lane);  // (lane 0's word is the entry point's key)
                lst.refresh_last(ef);
            } else {
                // p committed: marked where it sits NOW (its own keys may go in front of it), then c's and p's keys in
                // ONE merge -- the list is the ef smallest of the union either way (SURVEY.md N2)
                if (flags & 1u) {
                    if (is_p[0]) lst.L[0] |= LK_EXPANDED;
                    if constexpr (R == 2) {
                        if (is_p[1]) lst.L[1] |= LK_EXPANDED;
                    }
                }
                lst.merge((upper && !(flags & 1u)) ? LK_INVALID : key, ef, perm, lane);
            }
            PP_ADD(PAIR_K_MERGES, m0);
            [[maybe_unused]] const unsigned long long f0 = PP_NOW();
            // The list's four smallest unexpanded entries, written by the lanes that hold them (no read-lanes): the next
            // pass's c -- marked expanded here and now -- and p, and the two behind them.
            const bool ue0 = (int32_t)(uint32_t)(lst.L[0] >> 32) >= 0;
            const u64 U0 = __ballot(ue0);
            const uint32_t n0 = (uint32_t)__popcll(U0);
            const uint32_t r0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(U0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)U0, 0u));
            uint32_t nf = min(n0, 4u);
            if (ue0 && r0 < 4u) box->f_key[r0] = lst.L[0];
            is_p[0] = ue0 && r0 == 1u;
            if (ue0 && r0 == 0u) lst.L[0] |= LK_EXPANDED;
            if constexpr (R == 2) {
                is_p[1] = false;
                if (HX_UNLIKELY(n0 < 4u && lst.n_cur > 64u)) {
                    const bool ue1 = (int32_t)(uint32_t)(lst.L[1] >> 32) >= 0;
                    const u64 U1 = __ballot(ue1);
                    const uint32_t r1 = n0 + __builtin_amdgcn_mbcnt_hi((uint32_t)(U1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)U1, 0u));
                    nf = min(n0 + (uint32_t)__popcll(U1), 4u);
                    if (ue1 && r1 < 4u) box->f_key[r1] = lst.L[1];
                    is_p[1] = ue1 && r1 == 1u;
                    if (ue1 && r1 == 0u) lst.L[1] |= LK_EXPANDED;
                }
            }
            if (lane == 0) box->f_n = nf;
            asm volatile("" ::: "memory");
            box_store(&box->f_seq, k + 1u);  // F of pass k
            PP_ADD(PAIR_K_F, f0);
            if (nf == 0) break;  // candidates exhausted / only worse ones left (searcher.rs:35, 41-44)
        }
        // the walker's verdict, then get_top_selected(n) (results.rs:59-61)
        {
            bool done = false;
            for (uint32_t it = 0; it < PAIR_POLLS && !done; it++) {
                done = uni(box_load(&box->b_done)) != 0;
                if (!done) __builtin_amdgcn_s_sleep(1);
            }
            if (!done) status = HNSW_ERR_HIP;
        }
        const int32_t bst = (int32_t)uni(box_load(reinterpret_cast<const uint32_t *>(&box->b_status)));
        if (status == HNSW_OK) status = bst;
        const uint32_t count = status == HNSW_OK ? min(a.n, lst.n_cur) : 0;
        write_results(a, q, lst, count, lane);
        PP_WRITE_KEEPER();
        return;
    }

    // ============================== the walker ==============================
    __builtin_amdgcn_s_setprio(3);
    Visited vis;
    vis.tab = reinterpret_cast<uint32_t *>(smem);
    uint32_t n_dist = 0, n_exp = 0, sum_deg = 0, n_vis = 0;
    int32_t status = HNSW_OK;
    PP_STATE_WALKER();

    QueryRegs<DS> qreg;
    float(&qv)[DS] = qreg.v;
    if (!load_query_f32<DS>(a.Q + (size_t)q * DS, qv, lane)) status = HNSW_ERR_NAN_INPUT;

    // ---- entry point (template.rs:316-319) ----
    u64 best = LK_INVALID;
    uint32_t cur = a.ep;
    if (status == HNSW_OK) {
        if (cur >= a.n_points) {
            status = HNSW_ERR_ARG;
        } else {
            const float d0 = row_dist<DS>(a.rows, cur, lane == 0, qv);
            const uint32_t bits = rdlane(__builtin_bit_cast(uint32_t, d0), 0);
            n_dist = 1;
            if (__builtin_bit_cast(float, bits) != __builtin_bit_cast(float, bits))
                status = HNSW_ERR_NAN_INPUT;
            else
                best = ((u64)bits << 32) | cur;
        }
    }

    // ---- upper layers, ef = 1: the greedy walk of hx_lean_f32_kernel ----
    const uint32_t up_slots = max(hslots >> 2, 64u);
    uint32_t ub_cur = HX_EMPTY_SLOT;
    bool have_ub = false;
    for (int layer = (int)a.nb_layers - 1; layer >= 1 && status == HNSW_OK; layer--) {
        vis.bshift = 32 - (__ffs((int)up_slots) - 1 - 2);
        vis.bmask = (up_slots >> 2) - 1;
        const uint32_t vis_limit = up_slots - (up_slots >> 2);
        vis.clear(up_slots, lane);
        vis.insert(cur, lane == 0);
        n_vis = 1;
        if (!have_ub) {
            ub_cur = uni(a.upper_base[cur]);
            have_ub = true;
        }
        while (status == HNSW_OK) {
            if (ub_cur == HX_EMPTY_SLOT) {
                status = HNSW_ERR_NODE_NOT_IN_GRAPH;
                break;
            }
            n_exp++;
            bool improved = false;
            uint32_t new_cur = cur, new_ub = ub_cur;
            const uint32_t *row = a.adj_up + ((size_t)ub_cur + (uint32_t)layer - 1) * a.S1;
            uint32_t ovf_lo = 0, ovf_hi = 0;
            bool first = true;
            while (true) {
                uint32_t nb = HX_EMPTY_SLOT;
                if (first) {
                    if ((uint32_t)lane < a.S1) nb = row[lane];
                } else {
                    if (ovf_lo + lane < ovf_hi) nb = a.ovf_nbrs[ovf_lo + lane];
                    ovf_lo += 64;
                }
                const bool valid = (int32_t)nb >= 0;
                if (first) {
                    const u64 pm = __ballot((int32_t)nb < 0 && nb != HX_EMPTY_SLOT);
                    if (HX_UNLIKELY(pm != 0)) {
                        const uint32_t o = rdlane(nb, (uint32_t)__ffsll((long long)pm) - 1) & ~HX_OVF_FLAG;
                        ovf_lo = uni(a.ovf_off[o]);
                        ovf_hi = uni(a.ovf_off[o + 1]);
                    }
                    first = false;
                }
                const uint32_t cnt = (uint32_t)__popcll(__ballot(valid));
                sum_deg += cnt;
                if (HX_LIKELY(cnt != 0)) {
                    if (HX_UNLIKELY(n_vis + cnt > vis_limit)) {
                        status = HNSW_ERR_OVERFLOW;
                        break;
                    }
                    const bool fresh = vis.insert(nb, valid);
                    const u64 fm = __ballot(fresh);
                    const uint32_t nf = (uint32_t)__popcll(fm);
                    n_vis += nf;
                    n_dist += nf;
                    if (HX_LIKELY(fm != 0)) {
                        uint32_t ubn = HX_EMPTY_SLOT;
                        if (fresh) ubn = a.upper_base[nb];
                        const float dist = row_dist<DS>(a.rows, nb, fresh, qv);
                        const bool nan = fresh && dist != dist;
                        if (HX_UNLIKELY(__ballot(nan) != 0)) {
                            status = HNSW_ERR_NAN_INPUT;
                            break;
                        }
                        const uint32_t db = fresh ? __builtin_bit_cast(uint32_t, dist) : 0xFFFFFFFFu;
                        const uint32_t mn = wave_min_u32(db);
                        u64 tie = __ballot(fresh && db == mn);
                        uint32_t j = (uint32_t)__ffsll((long long)tie) - 1;
                        uint32_t bid = rdlane(nb, j);
                        tie &= tie - 1;
                        while (tie) {  // equal distances: the smaller id wins (dist.rs:30-38)
                            const uint32_t j2 = (uint32_t)__ffsll((long long)tie) - 1;
                            tie &= tie - 1;
                            const uint32_t id2 = rdlane(nb, j2);
                            if (id2 < bid) {
                                bid = id2;
                                j = j2;
                            }
                        }
                        const u64 kk = ((u64)mn << 32) | bid;
                        if (kk < best) {
                            best = kk;
                            new_cur = bid;
                            new_ub = rdlane(ubn, j);
                            improved = true;
                        }
                    }
                }
                if (HX_LIKELY(ovf_lo >= ovf_hi)) break;
            }
            if (!improved || status != HNSW_OK) break;
            cur = new_cur;
            ub_cur = new_ub;
        }
    }

    // ---- layer 0 with ef (template.rs:326) ----
    if (status == HNSW_OK) {
        const uint32_t vis_limit = layer0_table<false>(a, vis, hslots, cur, lane).all;
        n_vis = 1;  // the entry point: what layer0_table put into the emptied table
        box->keys[lane] = best;
        asm volatile("" ::: "memory");
        box_store(&box->k_seq, 1u);

        const uint32_t S0 = a.S0;
        const bool upper = lane >= 32;
        const uint32_t slot = (uint32_t)lane & 31u;
        uint32_t cid = cur, pid = HX_EMPTY_SLOT;
        uint32_t nb = HX_EMPTY_SLOT;  // the adjacency rows of (cid, pid): requested at the end of the pass before
        if (!upper && slot < S0) nb = a.adj0[(size_t)cid * S0 + slot];
        [[maybe_unused]] const unsigned long long t_l0 = PP_NOW();
        for (uint32_t k = 0;; k++) {
            [[maybe_unused]] const unsigned long long g0 = PP_NOW();
            PP_COUNT(PAIR_W_PASSES);
            // ---- the gather for (cid, pid): nothing of it is counted before the keeper's F confirms the pair ----
            const bool have_p = pid != HX_EMPTY_SLOT;
            if (HX_UNLIKELY(__ballot((int32_t)nb < -1) != 0)) {  // degree > S0: the one-wave kernel
                status = HX_PAIR_EXIT(2);
                break;
            }
            const bool valid = (int32_t)nb >= 0;
            const uint32_t vb = vis.home(nb);
            const uint32_t vt0 = vis.look(nb, vb);
            const uint32_t vt = valid ? vt0 : 4u;
            const bool want_pre = vt != 4u;
            const uint32_t ct = upper ? 4u : vt;
            bool fresh = false;
            float dist = 0.0f;
            if (want_pre) {
                const uint4 *src = reinterpret_cast<const uint4 *>(a.rows + (size_t)nb * DS);
                uint4 w[DS / 4];
#pragma unroll
                for (int p = 0; p < DS / 4; p++) w[p] = src[p];
                __builtin_amdgcn_sched_barrier(0);
                const uint32_t old = vis.claim(nb, vb, ct);
                fresh = old == HX_EMPTY_SLOT;
                const bool pend = (ct != 4u) & !fresh;
                if (HX_UNLIKELY(__ballot(pend) != 0)) fresh = vis.finish(nb, vb, ct, pend, fresh);
                __builtin_amdgcn_sched_barrier(0);
                const float s = chain_sum<DS>(w, qv);
                dist = __builtin_sqrtf(s);
            }
            const bool want = upper ? want_pre : fresh;
            const bool nan = want && dist != dist;
            u64 key = LK_INVALID;
            if (want && !nan) key = ((u64)__builtin_bit_cast(uint32_t, dist) << 32) | nb;
            const u64 vmask = __ballot(valid), fmask = __ballot(fresh);
            const uint32_t cnt_c = (uint32_t)__popcll(vmask & 0xFFFFFFFFull);
            const uint32_t cnt_p = (uint32_t)__popcll(vmask >> 32);
            const uint32_t nf_c = (uint32_t)__popcll(fmask);
            n_vis += nf_c;  // (the table holds them whether or not the pass counts)
            PP_ADD(PAIR_W_GATHER, g0);  // (look .. chain)
            [[maybe_unused]] const unsigned long long w0 = PP_NOW();

            // ---- the keeper's view of the list before this pass: the word first, F behind it, one round trip ----
            uint32_t nF = 0;
            u64 F0 = 0, F1 = 0, F2 = 0, F3 = 0;
            bool got = false;
            for (uint32_t it = 0; it < PAIR_POLLS; it++) {
                const uint32_t seq = box_load(&box->f_seq);
                nF = box_load(&box->f_n);
                F0 = box_load64(&box->f_key[0]);
                F1 = box_load64(&box->f_key[1]);
                F2 = box_load64(&box->f_key[2]);
                F3 = box_load64(&box->f_key[3]);
                const uint32_t ab = box_load(&box->abort);
                if (uni(seq) >= k + 1u) {
                    got = true;
                    break;
                }
                if (uni(ab) != 0) break;
                __builtin_amdgcn_s_sleep(1);
            }
            if (HX_UNLIKELY(!got)) {
                status = HNSW_ERR_HIP;
                break;
            }
            PP_ADD(PAIR_W_WAIT_F, w0);
            [[maybe_unused]] const unsigned long long c0 = PP_NOW();
            nF = uni(nF);
            if (nF == 0) break;  // the search is over; the gather above is dropped
            if (HX_UNLIKELY(uni((uint32_t)F0) != cid)) {  // (not known to happen: see the header)
                status = HX_PAIR_EXIT(3);
                break;
            }
            const bool p_ok = have_p && nF >= 2u && uni((uint32_t)F1) == pid;
            n_exp++;
            sum_deg += cnt_c;
            n_dist += nf_c;
            if (HX_UNLIKELY(n_vis > vis_limit)) {
                status = HNSW_ERR_OVERFLOW;
                break;
            }
            if (HX_UNLIKELY((__ballot(nan) & 0xFFFFFFFFull) != 0)) {
                status = HNSW_ERR_NAN_INPUT;  // Dist::cmp would panic (dist.rs:32)
                break;
            }
            // p is expanded in this pass when it is still the smallest unexpanded entry after c's keys went in
            const bool p_commits = p_ok && __ballot(!upper && key < F1) == 0;
            // ---- the next pair: the two smallest unexpanded keys there will be once the keeper has merged.  p's keys
            // are those its look called absent: the few that c inserted in this very pass appear twice and are skipped
            // (its claims, below, are exact).  The pair's adjacency rows are requested at once. ----
            // (A p lane whose home bucket was full cannot tell "absent" from "in a later bucket" before its claim: a pass
            // with such a lane decides after p's claims, on exact keys.)
            const bool late = p_commits && __ballot(upper && vt == 5u) != 0;
            PP_ADD(PAIR_W_CHECK, c0);
            uint32_t ncid = HX_EMPTY_SLOT, npid = HX_EMPTY_SLOT, nnb = HX_EMPTY_SLOT;
            auto next_pair = [&](u64 pk) __attribute__((always_inline)) {
                // The two smallest of the wave's keys by two wave-wide minima over the distance words (DPP; a loop over
                // the candidate lanes cost ~ 150 cycles per key and a pass has five to ten below F[3]), then the two
                // smallest of those and the list's own two, on scalars.
                const bool elig = pk != LK_INVALID && (p_commits || !upper);
                const uint32_t pd = (uint32_t)(pk >> 32), pi = (uint32_t)pk;
                auto min_of = [&](bool in, uint32_t &d, uint32_t &i) __attribute__((always_inline)) {
                    d = wave_min_u32(in ? pd : 0xFFFFFFFFu);
                    i = HX_EMPTY_SLOT;
                    if (d != 0xFFFFFFFFu) {
                        u64 tie = __ballot(in && pd == d);
                        i = rdlane(pi, (uint32_t)__ffsll((long long)tie) - 1);
                        tie &= tie - 1;
                        while (HX_UNLIKELY(tie != 0)) {  // equal distances: the smaller id first (dist.rs:30-38)
                            const uint32_t i2 = rdlane(pi, (uint32_t)__ffsll((long long)tie) - 1);
                            tie &= tie - 1;
                            i = min(i, i2);
                        }
                    }
                };
                const u64 b1 = p_commits ? (nF >= 3u ? F2 : LK_INVALID) : (nF >= 2u ? F1 : LK_INVALID);
                const u64 b2 = p_commits ? (nF >= 4u ? F3 : LK_INVALID) : (nF >= 3u ? F2 : LK_INVALID);
                const uint32_t b1d = uni((uint32_t)(b1 >> 32)), b1i = uni((uint32_t)b1), b2d = uni((uint32_t)(b2 >> 32)), b2i = uni((uint32_t)b2);
                auto less = [](uint32_t ad, uint32_t ai, uint32_t bd, uint32_t bi) { return ad < bd || (ad == bd && ai < bi); };
                // only keys below the list's second candidate matter: none (the converged part of a search) or one of
                // them needs no minimum over the wave
                const u64 below = __ballot(elig && pk < b2);
                uint32_t w1d = 0xFFFFFFFFu, w1i = HX_EMPTY_SLOT, w2d = 0xFFFFFFFFu, w2i = HX_EMPTY_SLOT;
                if (below != 0) {
                    if ((below & (below - 1)) == 0) {
                        const uint32_t j = (uint32_t)__ffsll((long long)below) - 1;
                        w1d = rdlane(pd, j);
                        w1i = rdlane(pi, j);
                    } else {
                        min_of(elig, w1d, w1i);
                        min_of(elig && pi != w1i, w2d, w2i);  // (p's lane may carry a key c inserted in this very pass: the same id)
                    }
                }
                // merge of the two sorted pairs (w1 <= w2, b1 <= b2): the first two
                uint32_t d1, i1, d2, i2;
                if (less(w1d, w1i, b1d, b1i)) {
                    d1 = w1d, i1 = w1i;
                    if (less(w2d, w2i, b1d, b1i)) d2 = w2d, i2 = w2i; else d2 = b1d, i2 = b1i;
                } else {
                    d1 = b1d, i1 = b1i;
                    if (less(w1d, w1i, b2d, b2i)) d2 = w1d, i2 = w1i; else d2 = b2d, i2 = b2i;
                }
                ncid = d1 != 0xFFFFFFFFu ? i1 : HX_EMPTY_SLOT;  // (all ones = none: a distance word is never that, NaNs are out)
                npid = d2 != 0xFFFFFFFFu ? i2 : HX_EMPTY_SLOT;
                if (ncid != HX_EMPTY_SLOT && slot < S0 && (!upper || npid != HX_EMPTY_SLOT)) nnb = a.adj0[(size_t)(upper ? npid : ncid) * S0 + slot];
            };
            // p's claims are requested first and looked at after the pick: the compare-and-swap's round trip runs under it
            const uint32_t pt = (upper && p_commits) ? vt : 4u;
            const uint32_t pold = vis.claim(nb, vb, pt);
            if (HX_LIKELY(!late)) next_pair(key);
            PP_ADD(PAIR_W_CHECK_NEXT, c0);
            [[maybe_unused]] const unsigned long long s0 = PP_NOW();
            bool pfresh = false;
            if (p_commits) {
                n_exp++;
                pfresh = pold == HX_EMPTY_SLOT;
                const bool ppend = (pt == 5u) | ((pt < 4u) & !pfresh & (pold != nb));
                if (HX_UNLIKELY(__ballot(ppend) != 0)) pfresh = vis.finish(nb, vb, pt == 5u ? 5u : 0u, ppend, pfresh);
                const uint32_t nf_p = (uint32_t)__popcll(__ballot(pfresh));
                sum_deg += cnt_p;
                n_vis += nf_p;
                n_dist += nf_p;
                if (HX_UNLIKELY(n_vis > vis_limit)) {
                    status = HNSW_ERR_OVERFLOW;
                    break;
                }
                if (HX_UNLIKELY(__ballot(pfresh && nan) != 0)) {
                    status = HNSW_ERR_NAN_INPUT;
                    break;
                }
            }
            if (HX_UNLIKELY(late)) next_pair(upper ? (pfresh ? key : LK_INVALID) : key);
            PP_ADD(PAIR_W_CLAIMS_P, s0);
            [[maybe_unused]] const unsigned long long n0 = PP_NOW();
            // ---- this pass's keys to the keeper (it took the previous ones out before it published this pass's F) ----
            box->keys[lane] = upper ? (pfresh ? key : LK_INVALID) : key;
            if (lane == 0) box->k_flags = p_commits ? 1u : 0u;
            asm volatile("" ::: "memory");
            box_store(&box->k_seq, k + 2u);
            __builtin_amdgcn_sched_barrier(0);  // (the copy below waits for the rows just requested: after the send, not before)
            PP_ADD(PAIR_W_SEND, n0);
            cid = ncid;
            pid = npid;
            nb = nnb;
        }
        PP_ADD(PAIR_W_LAYER0, t_l0);
    }
    if (status != HNSW_OK) box_store(&box->abort, 1u);
    PP_WRITE_WALKER();
    if (lane == 0) box->b_status = status;
    write_stats(a, q, n_dist, n_exp, sum_deg, status, lane);
    asm volatile("" ::: "memory");
    box_store(&box->b_done, 1u);
}

template <int DS, class LT>
int launch_pair(const LeanArgs &a, uint32_t nblocks, hipStream_t stream) {
    constexpr int R = LT::NR;
    const size_t lds = (4ull << a.slots_log2) + (64ull * R + 64) * 8 + sizeof(PairBox);
    return launch_checked({"search kernel launch", "search needs %zu bytes of LDS (> 160 KiB)"}, hx_pair_f32_kernel<DS, LT>,
                          dim3(nblocks), dim3(128), lds, stream, a);
}
