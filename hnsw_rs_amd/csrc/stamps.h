// stamps.h -- the in-kernel cycle stamps of the diagnostic build (make stamps; never shipped, never timed): per-phase
// cycle sums and event counts of one query, kept in registers and written once, at the query's end, to a side
// buffer nothing else reads (SearchArgs::dbg / LeanArgs::dbg, set from HX_DBG_PTR under HX_STAMPS alone).
//
// The layout of that buffer is stamp_slots.inc: HX_STAMP_STRIDE values per query for every kernel, every slot a name
// and a number.  A kernel names the event on one line; without HX_STAMPS every line here is empty and none of its
// arguments is evaluated, so the shipped kernels do not change with what is measured.  Slots are compile-time
// constants everywhere: a computed index would move the accumulators from registers to scratch.
//
// What a kernel needs for it: STAMP_STATE... once where its counters are declared, then the event lines, then its
// STAMP_WRITE... line.  The lines use the kernel's own `a`, `q` and `lane`.
#pragma once

#include "stamp_slots.inc"

namespace hx {

#define HX_STAMP_ENUM(list, NAME, number, desc) list##_##NAME = number,
enum StampSlot : int {
    HX_STAMP_SLOTS_LEAN(HX_STAMP_ENUM) HX_STAMP_SLOTS_MERGE(HX_STAMP_ENUM) HX_STAMP_SLOTS_Q8(HX_STAMP_ENUM)
        HX_STAMP_SLOTS_FAT(HX_STAMP_ENUM) HX_STAMP_SLOTS_GENERIC(HX_STAMP_ENUM) HX_STAMP_SLOTS_PAIR(HX_STAMP_ENUM)
};
#undef HX_STAMP_ENUM

#ifdef HX_STAMPS

// a stamp drains the wave's memory counters and is a scheduling barrier, so that what lies between two
// stamps is exactly the code written between them
__device__ __forceinline__ unsigned long long stamp_now() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const unsigned long long t = __builtin_readcyclecounter();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}

// ---- the accumulators and the clock at the kernel's start ----
#define STAMP_STATE()                                    \
    unsigned long long dbg_acc[HX_STAMP_STRIDE] = {};   \
    const unsigned long long t_begin = __builtin_readcyclecounter()
// one value of `list` from the registers to the query's part of the buffer (the write-outs below)
#define HX_STAMP_STORE(list, NAME, number, desc) a.dbg[(size_t)q * HX_STAMP_STRIDE + number] = dbg_acc[number];

// ---- the clock, two ways ----
// STAMP: stamp_now() (the lean kernels); STAMP_RAW: the counter as it is, nothing drained (hx_search_kernel, whose
// loops keep DMA and prefetches in flight across their stamps)
#define STAMP(var) const unsigned long long var = stamp_now()
#define STAMP_RAW(var) const unsigned long long var = __builtin_readcyclecounter()
// the clock once the LDS requests are back, whatever is still in flight from memory (stamp_now would wait for it)
#define STAMP_LDS(var)                                            \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           \
    const unsigned long long var = __builtin_readcyclecounter(); \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define STAMP_WAIT_VMEM() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

// ---- sums and counts ----
#define STAMP_ADD(slot, t0, t1) dbg_acc[slot] += (t1) - (t0)
#define STAMP_ADD_NOW(slot, t0) dbg_acc[slot] += stamp_now() - (t0)
#define STAMP_SINCE_BEGIN(slot) dbg_acc[slot] = __builtin_readcyclecounter() - t_begin
#define STAMP_COUNT(slot) dbg_acc[slot]++
#define STAMP_COUNT_N(slot, n) dbg_acc[slot] += (n)

// ---- hx_lean_f32_kernel ----
// the runner-up's misses (slots 16 .. 24): what the last miss predicted for the pass that follows it
#define STAMP_STATE_LEAN_F32()                              \
    STAMP_STATE();                                          \
    bool dbg_follow = false, dbg_took_pre = false;          \
    uint32_t dbg_pred_c = HX_EMPTY_SLOT, dbg_pred_p = HX_EMPTY_SLOT, dbg_old_p = HX_EMPTY_SLOT
// the frontier's run at the pick: F is kept live up to the stamp, so the run lies in front of it
#define STAMP_FRONTIER_AT_PICK(t0, F)                                                        \
    do {                                                                                     \
        asm volatile("" ::"v"((F)[0]), "v"((F)[1]), "v"((F)[2]), "v"((F)[3]) : "memory");  \
        STAMP_ADD_NOW(LEAN_FRONTIER, t0);                                                    \
        STAMP_COUNT(LEAN_FRONTIER_RUNS);                                                     \
    } while (0)
#define STAMP_FRONTIER_RERUN()              \
    do {                                    \
        STAMP_COUNT(LEAN_FRONTIER_RUNS);    \
        STAMP_COUNT(LEAN_FRONTIER_RERUNS);  \
    } while (0)
// the pick (cid, pid): was it what the last miss foresaw, and is it the pair whose rows were fetched ahead?
#define STAMP_NOTE_PICK(cid, pid, pre_c, pre_p)                                                 \
    do {                                                                                        \
        if (dbg_follow) {                                                                       \
            if ((cid) == dbg_pred_c && (pid) == dbg_pred_p) STAMP_COUNT(LEAN_MISS_PREDICTED);   \
            if ((pid) == dbg_old_p) STAMP_COUNT(LEAN_MISS_OLD_P);                               \
            dbg_follow = false;                                                                 \
        }                                                                                       \
        dbg_took_pre = (pre_c) == (cid) && (pre_p) == (pid);                                    \
    } while (0)
// a foreseen miss: bm c's fresh keys below p's key, (pred_c, pred_p) the pair requested for the next pass
#define STAMP_NOTE_MISS(bm, pred_c, pred_p, old_p)              \
    do {                                                        \
        const uint32_t nbel = (uint32_t)__popcll(bm);           \
        if (nbel == 1) STAMP_COUNT(LEAN_MISS_1);                \
        else if (nbel == 2) STAMP_COUNT(LEAN_MISS_2);           \
        else STAMP_COUNT(LEAN_MISS_3_UP);                       \
        dbg_follow = true;                                      \
        dbg_pred_c = (pred_c);                                  \
        dbg_pred_p = (pred_p);                                  \
        dbg_old_p = (old_p);                                    \
    } while (0)
// the pass has its rows' addresses: the adjacency round trip ends here
#define STAMP_PASS_PICKED()         \
    STAMP_WAIT_VMEM();              \
    STAMP_COUNT(LEAN_PASSES)
// slot 0 again on the passes that took the rows fetched ahead
#define STAMP_PICK_AHEAD(ovf_pass, t0, t1)      \
    do {                                        \
        if (!(ovf_pass) && dbg_took_pre) {      \
            STAMP_ADD(LEAN_PICK_AHEAD, t0, t1); \
            STAMP_COUNT(LEAN_PASSES_AHEAD);     \
        }                                       \
    } while (0)
// slot 1 again on the passes whose runner-up kept its distances
#define STAMP_FILTER_KEPT(kept, t0, t1)             \
    do {                                            \
        if (kept) {                                 \
            STAMP_ADD(LEAN_FILTER_KEPT, t0, t1);    \
            STAMP_COUNT(LEAN_PASSES_KEPT);          \
        }                                           \
    } while (0)
// what is left of the row round trip once the claims are done (t1 is declared: the chain starts there) ...
#define STAMP_ROW_WAIT(t1)                  \
    __builtin_amdgcn_sched_barrier(0);      \
    STAMP_LDS(t1##_lds);                    \
    STAMP(t1);                              \
    STAMP_ADD(LEAN_ROW_WAIT, t1##_lds, t1)
// ... then the chain alone, up to its result
#define STAMP_CHAIN(t1, dist)                          \
    do {                                               \
        asm volatile("" ::"v"(dist) : "memory");       \
        STAMP_ADD_NOW(LEAN_CHAIN, t1);                 \
    } while (0)
// a merge's size before it runs: `survives` is the lane's "my key goes in".  Static slots, see above.
#define STAMP_MERGE_SIZE(survives, small, small_keys)                           \
    do {                                                                        \
        const uint32_t mm = (uint32_t)__popcll(__ballot(survives));             \
        if (mm == 0) STAMP_COUNT(LEAN_MERGES_0);                                \
        else if (mm <= 2) STAMP_COUNT(LEAN_MERGES_1_2);                         \
        else STAMP_COUNT(LEAN_MERGES_3_UP);                                     \
        if (mm != 0 && mm <= HX_MERGE_SHIFT_MAX) {                              \
            STAMP_COUNT(small);                                                 \
            STAMP_COUNT_N(small_keys, mm);                                      \
        }                                                                       \
    } while (0)
// The write-out is three plain ascending loops over the table's ranges -- LEAN_PICK up to the F_ slots (the merges'
// splits lie inside), the F_ slots where the build fills them (their range has one position without a slot, which
// takes its zero), the frontier's three -- and not a statement per table line: stores in another order, the F_
// slots' zeros from the plain build, or a loop behind a generated predicate each gave the kernel's loop another
// register allocation (it keeps its counters in SGPRs and spills some to VGPR lanes) and 0.5 % more cycles per query.
// Like this the plain stamps build's d = 100 lean f32 kernels -- the ones the recorded profiles of DESIGN.md section 10
// are about -- differ from the ones those profiles saw in the write-out alone (7 to 19 assembly lines).  That holds for
// no other kernel: under stamps the quant8, the d = 128, the pair kernels and all of hx_search_kernel came out with
// another register allocation when their accumulators got the common stride, and their stamped figures do not
// compare with older ones (the generic two-row f32 loop: FILTER 7 % and MERGE_C 12 % lower, ROW_WAIT and CHAIN 3 to
// 4 % higher, profiles/stamps_refactor.txt).  The shipped build has no stamps and is the parent's, byte for byte.
#define HX_STAMP_STORE_RANGE(first, last) \
    for (int i = (first); i <= (last); i++) a.dbg[(size_t)q * HX_STAMP_STRIDE + i] = dbg_acc[i]
#define STAMP_WRITE_LEAN_F32()                                                  \
    if (lane == 0 && a.dbg) {                                                   \
        STAMP_SINCE_BEGIN(LEAN_TOTAL);                                          \
        HX_STAMP_STORE_RANGE(LEAN_PICK, LEAN_F_STAGING - 1);                    \
        FSTAMP_STORE_RANGE(LEAN_F_STAGING, LEAN_F_EXPANSIONS);                  \
        HX_STAMP_STORE_RANGE(LEAN_FRONTIER, LEAN_FRONTIER_RERUNS);              \
    }

// A merge's own split: the five MERGE values from `dbg` on (the f32 kernel passes its accumulators from LEAN_MERGE_C
// on for c's merge, from LEAN_MERGE_P on for p's; a caller without a side buffer passes nothing and its merges carry
// no stamp).
#define MERGE_DBG_PARAM , unsigned long long *dbg = nullptr
#define MERGE_DBG_ARG(first) , dbg_acc + (first)
#define MERGE_STAMP(var) const unsigned long long var = dbg ? stamp_now() : 0ull
#define MERGE_ADD(off, v)           \
    do {                            \
        if (dbg) dbg[off] += (v);   \
    } while (0)

// ---- hx_lean_q8_kernel ----
#define STAMP_WRITE_LEAN_Q8()                   \
    do {                                        \
        if (lane == 0 && a.dbg) {               \
            STAMP_SINCE_BEGIN(Q8_TOTAL);        \
            HX_STAMP_SLOTS_Q8(HX_STAMP_STORE)   \
        }                                       \
    } while (0)

// ---- hx_search_kernel: its two loops ----
// dbg_mid: the clock when the rows' pieces have landed, taken inside the distance routine
#define STAMP_STATE_GENERIC()   \
    STAMP_STATE();              \
    unsigned long long dbg_mid = 0
#define STAMP_ROWS_LANDED()     \
    STAMP_WAIT_VMEM();          \
    dbg_mid = __builtin_readcyclecounter()
// (a pass that evaluates nothing has no such moment: its gather is empty)
#define STAMP_ROWS_LANDED_DEFAULT(t) dbg_mid = (t)
#define STAMP_ADD_AROUND_ROWS_LANDED(before, after, t0, t1)     \
    STAMP_ADD(before, t0, dbg_mid);                             \
    STAMP_ADD(after, dbg_mid, t1)
// the inline-rows loop: did the prefetch predict this candidate?
#define STAMP_NOTE_HIT(hit)         \
    const bool dbg_hit = (hit);     \
    if (dbg_hit) STAMP_COUNT(FAT_HITS)
#define STAMP_ADD_BY_HIT(on_hit, on_miss, t0, t1)   \
    if (dbg_hit)                                    \
        STAMP_ADD(on_hit, t0, t1);                  \
    else                                            \
        STAMP_ADD(on_miss, t0, t1)
// (a query runs one of the two loops, and FAT's numbers are among GENERIC's: the total is slot 4 for both)
#define STAMP_WRITE_GENERIC()                       \
    do {                                            \
        if (lane == 0 && a.dbg) {                   \
            STAMP_SINCE_BEGIN(GENERIC_TOTAL);       \
            HX_STAMP_SLOTS_GENERIC(HX_STAMP_STORE)  \
        }                                           \
    } while (0)

// ---- hx_pair_f32_kernel: each of its two waves has accumulators of its own and writes its own slots ----
#define PP_STATE() unsigned long long pp[HX_STAMP_STRIDE] = {}
#define PP_STATE_WALKER()   \
    PP_STATE();             \
    const unsigned long long t_begin = __builtin_readcyclecounter()
#define PP_NOW() __builtin_readcyclecounter()
#define PP_ADD(slot, t0) pp[slot] += __builtin_readcyclecounter() - (t0)
#define PP_COUNT(slot) pp[slot]++
#define HX_STAMP_STORE_PP(NAME) a.dbg[(size_t)q * HX_STAMP_STRIDE + PAIR_##NAME] = pp[PAIR_##NAME]
#define PP_WRITE_KEEPER()                   \
    do {                                    \
        if (lane == 0 && a.dbg) {           \
            HX_STAMP_STORE_PP(K_WAIT_KEYS); \
            HX_STAMP_STORE_PP(K_MERGES);    \
            HX_STAMP_STORE_PP(K_F);         \
        }                                   \
    } while (0)
#define PP_WRITE_WALKER()                                               \
    do {                                                                \
        if (lane == 0 && a.dbg) {                                       \
            pp[PAIR_W_TOTAL] = __builtin_readcyclecounter() - t_begin;  \
            HX_STAMP_STORE_PP(W_GATHER);                                \
            HX_STAMP_STORE_PP(W_WAIT_F);                                \
            HX_STAMP_STORE_PP(W_CLAIMS_P);                              \
            HX_STAMP_STORE_PP(W_SEND);                                  \
            HX_STAMP_STORE_PP(W_CHECK_NEXT);                            \
            HX_STAMP_STORE_PP(W_LAYER0);                                \
            HX_STAMP_STORE_PP(W_PASSES);                                \
            HX_STAMP_STORE_PP(W_TOTAL);                                 \
            HX_STAMP_STORE_PP(W_CHECK);                                 \
        }                                                               \
    } while (0)

#else  // !HX_STAMPS: every line is empty

#define STAMP_STATE()
#define STAMP(var)
#define STAMP_RAW(var)
#define STAMP_LDS(var)
#define STAMP_WAIT_VMEM()
#define STAMP_ADD(slot, t0, t1)
#define STAMP_ADD_NOW(slot, t0)
#define STAMP_SINCE_BEGIN(slot)
#define STAMP_COUNT(slot)
#define STAMP_COUNT_N(slot, n)
#define STAMP_STATE_LEAN_F32()
#define STAMP_FRONTIER_AT_PICK(t0, F)
#define STAMP_FRONTIER_RERUN()
#define STAMP_NOTE_PICK(cid, pid, pre_c, pre_p)
#define STAMP_NOTE_MISS(bm, pred_c, pred_p, old_p)
#define STAMP_PASS_PICKED()
#define STAMP_PICK_AHEAD(ovf_pass, t0, t1)
#define STAMP_FILTER_KEPT(kept, t0, t1)
#define STAMP_ROW_WAIT(t1)
#define STAMP_CHAIN(t1, dist)
#define STAMP_MERGE_SIZE(survives, small, small_keys)
#define STAMP_WRITE_LEAN_F32()
#define MERGE_DBG_PARAM
#define MERGE_DBG_ARG(first)
#define MERGE_STAMP(var)
#define MERGE_ADD(off, v)
#define STAMP_WRITE_LEAN_Q8()
#define STAMP_STATE_GENERIC()
#define STAMP_ROWS_LANDED()
#define STAMP_ROWS_LANDED_DEFAULT(t)
#define STAMP_ADD_AROUND_ROWS_LANDED(before, after, t0, t1)
#define STAMP_NOTE_HIT(hit)
#define STAMP_ADD_BY_HIT(on_hit, on_miss, t0, t1)
#define STAMP_WRITE_GENERIC()
#define PP_STATE()
#define PP_STATE_WALKER()
#define PP_NOW() 0ull
#define PP_ADD(slot, t0)
#define PP_COUNT(slot)
#define PP_WRITE_KEEPER()
#define PP_WRITE_WALKER()

#endif

// (make stamps EXTRA=-DHX_STAMPS_FRONT) the front of the lean f32 query split further, the F_ slots: its stamps
// lengthen slot 7 by a fifth, so the plain stamps build, whose slot 7 the recorded profiles compare, does without them
#if defined(HX_STAMPS) && defined(HX_STAMPS_FRONT)
#define FSTAMP(var) STAMP(var)
#define FSTAMP_LDS(var) STAMP_LDS(var)
#define FSTAMP_ADD(slot, t0, t1) STAMP_ADD(slot, t0, t1)
#define FSTAMP_COUNT(slot) STAMP_COUNT(slot)
#define FSTAMP_SINCE_BEGIN(slot) STAMP_SINCE_BEGIN(slot)
#define FSTAMP_STORE_RANGE(first, last) HX_STAMP_STORE_RANGE(first, last)
#else
#define FSTAMP(var)
#define FSTAMP_LDS(var)
#define FSTAMP_ADD(slot, t0, t1)
#define FSTAMP_COUNT(slot)
#define FSTAMP_SINCE_BEGIN(slot)
#define FSTAMP_STORE_RANGE(first, last)
#endif

}  // namespace hx
