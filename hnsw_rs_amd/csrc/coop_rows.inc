// coop_rows.inc -- included inside namespace hx by search_common.h, once (the kernel files and the standalone check
// scripts/micro/coop_rows_check.hip get it from there): the cooperative whole-line gather of wide FullVec rows.
// ---------------------------------------------------------------------------------------------
// FullVec rows of whole 128-byte lines (d a multiple of 32: 128, 256, 768), gathered COOPERATIVELY.
//
// Why: with one lane per row and 16 bytes per load, a wave instruction touches 64 different cache lines
// for 16 bytes each, and every line is asked for by eight consecutive instructions.  On a table far
// beyond the caches that shape tops out at 1.2 TB/s whatever the row size or the bytes in flight, while
// the SAME rows read eight lanes to a 128-byte line run at 5.8-6.9 TB/s on a 69-GB table
// (scripts/micro/footprint_gather.hip, profiles/r03_gather_shapes_*.txt; the measured HBM traffic of
// the lane-per-row shape is 1.0-1.1 x its bytes, so it is the request path per line, not over-fetch).
//
// How: the wave's wanted rows are ranked (rank = wanted lanes below); a load instruction covers stage s
// (128 bytes) of eight rows -- lane (g, t) = (lane / 8, lane % 8) reads bytes [16 t, 16 t + 16) of the
// stage for the row of rank 8 i + g -- and K stages of 4 instructions (32 rows) are in flight in
// registers.  A landed stage goes through a 4-KiB LDS image (ds_write_b128, 16-byte pieces XOR-swizzled
// so that the row-per-lane read below is conflict-free), from which the OWNER lane of each row reads its
// 128 bytes and continues its own sum.  The arithmetic is untouched: every row is still one lane's single
// left-to-right chain over all d elements (full.rs:23-29), only the bytes arrive by another road.  More
// than 32 wanted rows take a second round of the same loop (ranks 32..63).
//
// ids_s: 64 words of LDS scratch (rank -> row id); img: the 4-KiB stage image, 16-byte aligned.
// Returns the lane's sum (0 for a lane that wants nothing); all 64 lanes must call it together.
// ---------------------------------------------------------------------------------------------
// which search-kernel instantiations gather their rows this way (HX_COOP=0 at build time: the lane-per-row
// loops of round 2, for A/B runs)
#ifndef HX_COOP
#define HX_COOP 1
#endif
template <int KIND, int DS>
__host__ __device__ constexpr bool coop_rows() {
    return HX_COOP != 0 && KIND == HNSW_VEC_F32 && DS >= 128 && DS % 32 == 0;
}
constexpr size_t HX_COOP_IMG_BYTES = 4096;

#ifndef HX_COOP_K
#define HX_COOP_K 4  // stages of 128 B x 32 rows in flight, 4 loads per lane each (measured at 10M x 768d, efSearch 128:
                    // K = 4 2.37 ms per batch, 8 2.39 ms, 12 3.40 ms: profiles/r03_config2_coop_stage_depth.txt)
#endif
// yq: the query's values, anything indexable by element -- a pointer into LDS, or a register-resident copy
// (QueryRegs below) when UNROLL makes every stage index a compile-time constant.
template <int N>
struct QueryRegs {
    float v[N];
    __device__ __forceinline__ float operator[](int e) const { return v[e]; }
};
// One round: every wanted row (at most 512 / SB of them) goes through all of its stages.  LPR lanes read one
// stage (SB = 16 LPR bytes) of one row per instruction: 8 lanes = a whole 128-byte line, 32 rows per stage;
// 4 lanes = half a line, 64 rows per stage (each line is then asked for by two instructions instead of one --
// against eight for a lane per row).  The image is 4 KiB either way.
template <int DS, int K, int LPR, bool UNROLL, class Q>
__device__ __forceinline__ float f32_rows_coop_round(const uint8_t *rows, bool active, uint32_t rank, uint32_t nw,
                                                     const Q &yq, const uint32_t *ids_s, unsigned char *img, int lane) {
    // native vectors: a HIP uint4 is a struct, and copying one from the register ring to LDS is a memcpy
    // that keeps the whole ring in scratch
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    constexpr int SB = 16 * LPR;                  // bytes of a row per stage
    constexpr int PPS = LPR;                      // 16-byte pieces per stage and row
    constexpr int RPI = 64 / LPR;                 // rows per load instruction
    constexpr int NS = DS * 4 / SB;               // stages per row
    constexpr int KK = K < NS ? K : NS;           // stages in flight
    static_assert(NS % KK == 0, "the stage ring divides the row");
    constexpr size_t ROWB = (size_t)DS * 4;
    // XOR swizzle of the pieces inside a row's stage: rows that share a 16-lane ds_read_b128 group then read
    // 16 different 16-byte slots of the 256-byte bank row
    constexpr uint32_t SWS = LPR == 8 ? 1 : 2, SWM = LPR - 1;
    const uint32_t g = (uint32_t)lane / LPR, t = (uint32_t)lane % LPR;
    float s = 0.0f;
    // rows of instruction i: rank RPI i + g; a rank past the end repeats the last row (the same line again: no
    // exec masks in the stream, no new traffic)
    const uint8_t *src[4];
    uint32_t wofs[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t slot = (uint32_t)RPI * i + g;
        const uint32_t rr = min(slot, nw - 1);
        src[i] = rows + (size_t)ids_s[rr] * ROWB + 16u * t;
        wofs[i] = slot * SB + ((t ^ ((slot >> SWS) & SWM)) << 4);
    }
    const bool mine = active;
    const unsigned char *rd = img + rank * SB;
    const uint32_t sw = (rank >> SWS) & SWM;
    u32x4 w[KK][4];
    // stage st of the ring slot j: image written, (slot refilled with stage st + KK,) owners sum
    auto to_image = [&](int j) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; i++) *reinterpret_cast<u32x4 *>(img + wofs[i]) = w[j][i];
    };
    auto request = [&](int j, int st) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; i++) w[j][i] = *reinterpret_cast<const u32x4 *>(src[i] + SB * st);
    };
    auto owners_sum = [&](int st) __attribute__((always_inline)) {
        if (mine) {
            const int y0 = 4 * PPS * st;
#pragma unroll
            for (int k = 0; k < PPS; k++) {
                // (read as a HIP uint4: indexing a native 4-vector loaded from this swizzled address made
                // hipcc 7.2 fetch one dword per piece and splat it -- caught by scripts/micro/coop_rows_check.hip)
                const uint4 pp = *reinterpret_cast<const uint4 *>(rd + (((uint32_t)k ^ sw) << 4));
                // both pairs of a piece go through x - y and the square before the four adds that continue
                // the chain: a packed result consumed by the very next instruction costs a wait state
                const f32x2 xa = {__builtin_bit_cast(float, pp.x), __builtin_bit_cast(float, pp.y)};
                const f32x2 xb = {__builtin_bit_cast(float, pp.z), __builtin_bit_cast(float, pp.w)};
                const f32x2 ya = {yq[y0 + 4 * k], yq[y0 + 4 * k + 1]}, yb = {yq[y0 + 4 * k + 2], yq[y0 + 4 * k + 3]};
                const f32x2 da = xa - ya, db = xb - yb;
                const f32x2 qa = da * da, qb = db * db;
                s += qa.x;
                s += qa.y;
                s += qb.x;
                s += qb.y;
            }
        }
        // the next stage's image may only be written once every owner has read this one: one wave's
        // LDS operations execute in issue order, the clobber keeps the compiler from moving them across
        asm volatile("" ::: "memory");
    };
#pragma unroll
    for (int j = 0; j < KK; j++) request(j, j);
    if constexpr (UNROLL) {
#pragma unroll
        for (int st0 = 0; st0 + KK < NS; st0 += KK) {
#pragma unroll
            for (int j = 0; j < KK; j++) {
                to_image(j);
                request(j, st0 + KK + j);
                owners_sum(st0 + j);
            }
        }
    } else {
#pragma unroll 1
        for (int st0 = 0; st0 + KK < NS; st0 += KK) {  // every slot is refilled
#pragma unroll
            for (int j = 0; j < KK; j++) {
                to_image(j);
                request(j, st0 + KK + j);
                owners_sum(st0 + j);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < KK; j++) {  // the last KK stages
        to_image(j);
        owners_sum(NS - KK + j);
    }
    return s;
}

#ifndef HX_COOP_HALF_LINES
#define HX_COOP_HALF_LINES 1  // 0: two eight-lane rounds for more than 32 rows (round 3's first form), for A/B runs
#endif
template <int DS, int K, bool UNROLL = false, bool HALF_LINES = (HX_COOP_HALF_LINES != 0), class Q = const float *>
__device__ __forceinline__ float f32_rows_coop(const uint8_t *rows, uint32_t id, bool active, const Q &yq,
                                               uint32_t *ids_s, unsigned char *img, int lane) {
    static_assert(DS % 32 == 0, "whole 128-byte lines");
    const u64 W = __ballot(active);
    const uint32_t nw = (uint32_t)__popcll(W);
    if (nw == 0) return 0.0f;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(W >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)W, 0u));
    if (active) ids_s[rank] = id;
    // up to 32 wanted rows: eight lanes to a 128-byte line.  33 to 64 (the candidate's and the runner-up's rows
    // together): four lanes to a half line, so that ONE round still serves every row -- a second round of the
    // eight-lane form would issue the whole chain's instructions again for a handful of rows.
    if constexpr (HALF_LINES) {
        if (nw <= 32) return f32_rows_coop_round<DS, K, 8, UNROLL>(rows, active, rank, nw, yq, ids_s, img, lane);
        return f32_rows_coop_round<DS, K, 4, UNROLL>(rows, active, rank, nw, yq, ids_s, img, lane);
    } else {
        // a second round of the eight-lane form for ranks 32 ..: the kernels whose registers do not hold both forms
        float s = 0.0f;
#pragma unroll 1
        for (uint32_t r0 = 0; r0 < nw; r0 += 32) {  // (one copy of the round's code)
            const bool mine = active && rank >= r0 && rank < r0 + 32;
            const float sr = f32_rows_coop_round<DS, K, 8, UNROLL>(rows, mine, (rank - r0) & 31u, min(nw - r0, 32u), yq,
                                                                   ids_s + r0, img, lane);
            s = mine ? sr : s;
        }
        return s;
    }
}

