// switches.h -- every environment switch of the library, and the only place under csrc/ that calls getenv.
// One accessor per switch; above each: what it means, its default, and when it is read.  "latched" is read at the
// accessor's first call and holds for the life of the process; "live" is read at every call, so a test may set it
// between two calls of the library.  A variable not named here is ignored.  Host code; include from anywhere.
#pragma once

#include <cstdint>
#include <cstdlib>

namespace hx {
namespace sw {

// the variable as a decimal integer (base 0: 0x.. too), `unset` where it is absent
inline long long env_int(const char *name, long long unset, int base = 10) {
    const char *e = getenv(name);
    return e ? strtoll(e, nullptr, base) : unset;
}
inline bool on_unless_0(const char *name) { return env_int(name, 1) != 0; }
inline bool off_unless_set(const char *name) { return env_int(name, 0) != 0; }

// ---- search: which kernel serves a launch (A/B runs) ----
// the lean kernels (search_lean.hip) serve the searches they are built for.  Default on.  Latched.
inline bool lean() { static const bool v = on_unless_0("HNSW_MI355X_LEAN"); return v; }
// ... 8-bit rows at d = 100 among them.  Default on.  Latched.
inline bool lean_q8() { static const bool v = on_unless_0("HNSW_MI355X_LEAN_Q8"); return v; }
// ... f32 rows at d = 128 (the cooperative gather) among them.  Default on.  Latched.
inline bool lean_128() { static const bool v = on_unless_0("HNSW_MI355X_LEAN_128"); return v; }
// ... lists of more than two registers (ef > 128) among them.  Default on.  Latched.
inline bool lean_wide() { static const bool v = on_unless_0("HNSW_MI355X_LEAN_WIDE"); return v; }
// ... and for 8-bit rows lists of five to eight registers (256 < ef <= 512).  Default on.  Latched.
inline bool lean_q8_wide() { static const bool v = on_unless_0("HNSW_MI355X_LEAN_Q8_WIDE"); return v; }
// The lean 8-bit kernel is enabled: what the dispatch (lean_applicable) and the choice of layout
// (DeviceIndex::wants_inline_rows) both ask, so that they cannot disagree within a process.
inline bool lean_q8_enabled() { return lean() && lean_q8(); }
// two waves per query (pair_kernel.inc) for f32 rows at d = 100, ef <= 128.  Default 0 (off).  Latched.
inline int pair_mode() { static const int v = (int)env_int("HNSW_MI355X_PAIR", 0); return v; }
// turns the two-rows-per-pass f32 loop of hx_search_kernel off; the lean kernels stand back.  Default off.  Latched.
inline bool one_row() { static const bool v = off_unless_set("HNSW_MI355X_ONE_ROW"); return v; }
// the HBM level of the two-level visited set (VisitedSpill, launch.h).  Default on.  Latched.
inline bool visited_2l() { static const bool v = on_unless_0("HNSW_MI355X_VISITED_2L"); return v; }
// ids after which the LDS level of that set closes (tests).  Default: `unset`, the kernel's own limit.  Live.
inline uint32_t visited_2l_limit(uint32_t unset) { return (uint32_t)env_int("HNSW_MI355X_VISITED_2L_LIMIT", unset); }

// ---- refined search ----
// the refinement gathers every width of table row with a lane per row, never cooperatively (A/B runs).  Default off.  Live.
inline bool refine_lane_rows() { return off_unless_set("HNSW_MI355X_REFINE_LANE_ROWS"); }

// ---- the HBM snapshot ----
// inline rows for 8-bit indexes: 1 builds them, 0 never does.  Default -1: the handle's own setting.  Live.
inline int inline_rows(int unset) { return (int)env_int("HNSW_MI355X_INLINE_ROWS", unset); }
// behave as if the host refused to pin memory: plain staging buffers, blocking copies (tests).  Default off.  Live.
inline bool no_pinned() { return off_unless_set("HNSW_MI355X_NO_PINNED"); }
// throw the snapshot away after an insertion or a build instead of patching it.  Default off.  Live.
inline bool reupload() { return off_unless_set("HNSW_MI355X_REUPLOAD"); }
// MiB of one upload staging piece; 0 or less: the built-in 64.  Default 0.  Latched.
inline long upload_piece_mb() { static const long v = (long)env_int("HNSW_MI355X_UPLOAD_PIECE_MB", 0); return v; }

// ---- host-pointer search ----
// small calls read queries and write results through mapped pinned memory, without copies.  Default on.  Latched.
inline bool zero_copy() { static const bool v = on_unless_0("HNSW_MI355X_ZERO_COPY"); return v; }
// ... up to this many queries per call.  Default 512.  Latched.
inline uint64_t zero_copy_max() { static const uint64_t v = (uint64_t)env_int("HNSW_MI355X_ZERO_COPY_MAX", 512, 0); return v; }

// ---- on-device build ----
// first-attempt size of the insert kernel's visited table, as a shift of the standard one (A/B runs, tests).
// Default: `unset`, the build's own rule.  Live.
inline int insert_table_adjust(int unset) { return (int)env_int("HNSW_MI355X_INSERT_TABLE_ADJUST", unset); }
// a sharded build connects on the rank that owns the row.  Default on.  Latched.
inline bool shard_connect() { static const bool v = on_unless_0("HNSW_MI355X_SHARD_CONNECT"); return v; }
// keep the edges' distances beside the adjacency for the length of a build.  Default on.  Latched.
inline bool build_edge_dists() { static const bool v = on_unless_0("HNSW_MI355X_BUILD_EDGE_DISTS"); return v; }

// ---- the stamps build (make stamps) only ----
// device address of the side buffer the cycle stamps go to.  Default 0: none.  Live.
inline unsigned long long dbg_ptr() { const char *e = getenv("HX_DBG_PTR"); return e ? strtoull(e, nullptr, 0) : 0; }

}  // namespace sw
}  // namespace hx
