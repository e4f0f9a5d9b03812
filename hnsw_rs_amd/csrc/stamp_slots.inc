// stamp_slots.inc -- the side buffer of the stamps build (make stamps), one line per slot:
//     X(list, NAME, number, "what the slot sums or counts")
// A query's part of the buffer is HX_STAMP_STRIDE values whichever kernel serves it; a kernel writes its own slots and
// the rest stay as the caller left them (the scripts allocate zeros).  stamps.h makes the enumerators (LEAN_PICK = 0, ...) from
// these lists and scripts/stamp_slots.py reads them by regular expression: keep one X(...) per line, the number a
// plain decimal literal, the description one string.  The numbers are the historical ones: DESIGN.md section 10 and
// the files under profiles/ cite slots by number, so a new slot takes a free number and no slot is renumbered.
//
// The lists: LEAN hx_lean_f32_kernel, Q8 hx_lean_q8_kernel, PAIR hx_pair_f32_kernel (its two waves), and the two
// loops of hx_search_kernel, which use the same numbers for different things: FAT the inline-rows loop
// (scripts/stamps.py), GENERIC the two-rows-per-pass f32 loop (scripts/stamps_f32.py).  MERGE is no kernel: the
// five offsets of a merge's own split, from the base the caller names (LEAN_MERGE_C, LEAN_MERGE_P).

#define HX_STAMP_STRIDE 64

#define HX_STAMP_SLOTS_LEAN(X)                                                                                  \
    X(LEAN, PICK, 0, "pick c,p + adjacency row round trip")                                                     \
    X(LEAN, FILTER, 1, "visited: insert c, look up p")                                                          \
    X(LEAN, ROW_WAIT, 2, "row gather until landed")                                                             \
    X(LEAN, CHAIN, 3, "chain + sqrt + key")                                                                     \
    X(LEAN, TOTAL, 4, "TOTAL (whole query)")                                                                    \
    X(LEAN, COMMIT_P, 5, "commit p: mark + visited insert")                                                     \
    X(LEAN, PASSES, 6, "layer-0 passes (count)")                                                                \
    X(LEAN, FRONT, 7, "staging + entry + upper layers")                                                         \
    X(LEAN, MERGE_C_ALL, 8, "merge c")                                                                          \
    X(LEAN, IS_P_NEXT, 9, "overflow rows + pick + is-p-next")                                                   \
    X(LEAN, MERGE_P_ALL, 10, "commit p: merge + pick")                                                          \
    X(LEAN, SLOW_ROUNDS, 11, "visited slow-loop rounds: passes with a second claim round (count)")              \
    X(LEAN, MERGES_0, 12, "merges with no survivor (count)")                                                    \
    X(LEAN, MERGES_1_2, 13, "merges with one or two survivors (count)")                                         \
    X(LEAN, MERGES_3_UP, 14, "merges with three or more survivors (count)")                                     \
    X(LEAN, P_COMMITS, 15, "p commits (count)")                                                                 \
    X(LEAN, MISS_1, 16, "runner-up misses with one fresh key of c below p (count)")                             \
    X(LEAN, MISS_2, 17, "runner-up misses with two fresh keys of c below p (count)")                            \
    X(LEAN, MISS_3_UP, 18, "runner-up misses with three or more fresh keys of c below p (count)")               \
    X(LEAN, MISS_PREDICTED, 19, "misses whose follow-up pick is the predicted pair (count)")                    \
    X(LEAN, MISS_OLD_P, 20, "misses whose follow-up runner-up is the old p (count)")                            \
    X(LEAN, PICK_AHEAD, 21, "slot 0 on the passes whose rows were fetched ahead")                               \
    X(LEAN, PASSES_AHEAD, 22, "passes that took rows fetched ahead (count)")                                    \
    X(LEAN, FILTER_KEPT, 23, "slot 1 on the passes whose runner-up kept its distances")                         \
    X(LEAN, PASSES_KEPT, 24, "passes whose runner-up kept its distances (count)")                               \
    X(LEAN, ENTRY, 25, "staging + entry point alone (slot 7 minus this: the walk)")                             \
    X(LEAN, MERGE_C, 26, "base of the split of c's merge: five values, see MERGE")                              \
    X(LEAN, MERGE_P, 31, "base of the split of p's merge: five values, see MERGE")                              \
    X(LEAN, SMALL_C, 36, "c's small merges, the ones that took the shift path (count)")                         \
    X(LEAN, SMALL_C_KEYS, 37, "keys c's small merges inserted (count)")                                         \
    X(LEAN, SMALL_P, 38, "p's small merges (count)")                                                            \
    X(LEAN, SMALL_P_KEYS, 39, "keys p's small merges inserted (count)")                                         \
    X(LEAN, F_STAGING, 40, "HX_STAMPS_FRONT: query staging alone")                                              \
    X(LEAN, F_CLEAR, 41, "HX_STAMPS_FRONT: the per-layer clear of the visited table")                           \
    X(LEAN, F_ROW_WAIT, 42, "HX_STAMPS_FRONT: what is left of the wait for the row an upper expansion takes")   \
    X(LEAN, F_FILTER, 43, "HX_STAMPS_FRONT: upper layers, look + claims")                                       \
    X(LEAN, F_ROWS_LEFT, 44, "HX_STAMPS_FRONT: upper layers, row round trip left once the filter is done")      \
    X(LEAN, F_CHAIN, 45, "HX_STAMPS_FRONT: upper layers, chain")                                                \
    X(LEAN, F_TABLE, 47, "HX_STAMPS_FRONT: layer-0 table set-up")                                               \
    X(LEAN, F_EXPANSIONS, 48, "HX_STAMPS_FRONT: upper-layer expansions (count)")                                \
    X(LEAN, FRONTIER, 50, "the frontier at the pick (inside slot 0, which its own stamp lengthens)")            \
    X(LEAN, FRONTIER_RUNS, 51, "frontier runs (count)")                                                         \
    X(LEAN, FRONTIER_RERUNS, 52, "frontier runs after c's merge: a survivor went in front of b (count)")

#define HX_STAMP_SLOTS_MERGE(X)                                             \
    X(MERGE, LOOP, 0, "survivor loop of the big merges")                    \
    X(MERGE, LDS, 1, "LDS phase: scatter, read back, holes, refresh_last")  \
    X(MERGE, SHIFT, 2, "shift path of the small merges")                    \
    X(MERGE, SURVIVORS, 3, "survivors of the big merges (count)")           \
    X(MERGE, BIG, 4, "big merges (count)")

#define HX_STAMP_SLOTS_Q8(X)                                            \
    X(Q8, PICK, 0, "pick + adjacency row (prefetch waited for here)")   \
    X(Q8, FILTER, 1, "visited look + claim + counts")                   \
    X(Q8, CHAIN, 3, "rows + chain + key")                               \
    X(Q8, TOTAL, 4, "TOTAL (whole query)")                              \
    X(Q8, PASSES, 6, "layer-0 passes (count)")                          \
    X(Q8, FRONT, 7, "staging + entry + upper layers")                   \
    X(Q8, MERGE, 8, "merge")

#define HX_STAMP_SLOTS_FAT(X)                                                       \
    X(FAT, PICK, 0, "pick+block (hit: LDS image, miss: HBM)+predict+DMA issue")     \
    X(FAT, FILTER_HIT, 1, "id+visited on prediction HITS (total)")                  \
    X(FAT, CHAIN, 2, "distance")                                                    \
    X(FAT, MERGE, 3, "merge")                                                       \
    X(FAT, TOTAL, 4, "TOTAL")                                                       \
    X(FAT, FILTER_MISS, 5, "id+visited on prediction MISSES (total)")               \
    X(FAT, HITS, 6, "prediction hits (count)")

#define HX_STAMP_SLOTS_GENERIC(X)                                           \
    X(GENERIC, PICK, 0, "pick c,p + adjacency row round trip")              \
    X(GENERIC, FILTER, 1, "visited: insert c, look up p")                   \
    X(GENERIC, ROW_WAIT, 2, "row gather until all 25 pieces landed")        \
    X(GENERIC, CHAIN, 3, "chain + sqrt")                                    \
    X(GENERIC, TOTAL, 4, "TOTAL (whole query)")                             \
    X(GENERIC, MERGE_C, 5, "merge c")                                       \
    X(GENERIC, COMMIT_P, 6, "pick + commit p (filter + merge)")             \
    X(GENERIC, PASSES, 7, "passes (count)")

#define HX_STAMP_SLOTS_PAIR(X)                                      \
    X(PAIR, W_GATHER, 0, "walker: gather (look .. chain)")          \
    X(PAIR, W_WAIT_F, 1, "walker: waiting for F")                   \
    X(PAIR, W_CLAIMS_P, 2, "walker: claims of p")                   \
    X(PAIR, W_SEND, 3, "walker: send")                              \
    X(PAIR, W_CHECK_NEXT, 4, "walker: check + next pair")           \
    X(PAIR, W_LAYER0, 5, "walker: layer 0")                         \
    X(PAIR, W_PASSES, 6, "walker: layer-0 passes (count)")          \
    X(PAIR, W_TOTAL, 7, "walker: TOTAL (whole query)")              \
    X(PAIR, K_WAIT_KEYS, 8, "keeper: waiting for keys")             \
    X(PAIR, K_MERGES, 9, "keeper: merges")                          \
    X(PAIR, K_F, 10, "keeper: F")                                   \
    X(PAIR, W_CHECK, 11, "walker: check alone")
