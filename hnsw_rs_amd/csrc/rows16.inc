// rows16.inc -- included inside namespace hx by search_rows16.hip and search_filtered16.hip, after search_common.h: how a row stored as IEEE
// binary16 ("rows_f16", DESIGN.md section 36) reaches its sum.  The arithmetic is FullVec's (full.rs:23-29) on the row
// widened back to f32: every row is one lane's single left-to-right f32 chain over all d elements, x = (float)h (exact),
// t = x - y, t = t * t, s = s + t, no contraction (-ffp-contract=off), and the caller takes the correctly rounded square
// root.  Only the bytes differ from the f32 kernels: 2 per element, eight elements per 16-byte piece, 64 per line.
//
// Widening: v_cvt_f32_f16 is exact for every binary16 value; a binary16 subnormal becomes a NORMAL f32 (m * 2^-24), and
// whether the instruction sees its input as a subnormal at all is the f64/f16 half of the wave's denormal mode, which
// hipcc leaves at "preserve" whatever is asked for f32.  tests/test_gpu_rows_f16.py holds rows of subnormals to the oracle.
// ---------------------------------------------------------------------------------------------
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));

// the eight elements of one 16-byte piece against y[0..8), continuing the chain s: difference and square of the whole
// piece before the eight adds (the source-order lesson of DESIGN.md section 4c: a result consumed by the very next
// instruction costs a wait state, and the adds are the chain)
__device__ __forceinline__ float f16_piece_fold(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, const float *y, float s) {
    const uint32_t w[4] = {w0, w1, w2, w3};
    float t[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const f16x2_t hh = __builtin_bit_cast(f16x2_t, w[i]);
        const float d0 = (float)hh.x - y[2 * i], d1 = (float)hh.y - y[2 * i + 1];
        t[2 * i] = d0 * d0;
        t[2 * i + 1] = d1 * d1;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) s += t[j];
    return s;
}
// the same for a piece that holds the row's end: elements at and beyond n_in (0 .. 8) are padding and add +0.0, which
// leaves a non-negative sum as it is
__device__ __forceinline__ float f16_piece_fold_tail(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, const float *y,
                                                     uint32_t n_in, float s) {
    const uint32_t w[4] = {w0, w1, w2, w3};
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const f16x2_t hh = __builtin_bit_cast(f16x2_t, w[j >> 1]);
        const bool in = (uint32_t)j < n_in;
        const float x = (float)((j & 1) ? hh.y : hh.x);
        const float d = x - (in ? y[j] : 0.0f);
        const float t = d * d;
        s += in ? t : 0.0f;
    }
    return s;
}

// ---------------------------------------------------------------------------------------------
// Any dimension: a lane per row.  The row is np = row_stride / 16 pieces (the last one zero-padded when d % 8 != 0; d < 8
// is one padded piece), streamed in stages of eight pieces -- 64 elements, one line -- through two register buffers, the
// next stage in flight while the current one is summed.  Every bound is wave-uniform (d is), so a stage past the row's
// end costs nothing and only the stage that holds the end takes the predicated fold.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float f16_row_lane(const uint8_t *row, uint32_t d, uint32_t np, const float *yq) {
    constexpr uint32_t CH = 8;
    const u32x4 *src = reinterpret_cast<const u32x4 *>(row);
    const uint32_t nst = (np + CH - 1) / CH;
    u32x4 a[CH], b[CH];
    auto fetch = [&](u32x4 (&w)[CH], uint32_t st) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t i = 0; i < CH; i++) {
            const u32x4 zero = {0u, 0u, 0u, 0u};
            w[i] = (st * CH + i < np) ? src[st * CH + i] : zero;
        }
    };
    auto fold = [&](const u32x4 (&w)[CH], uint32_t st, float s) __attribute__((always_inline)) -> float {
        const uint32_t e0 = 8 * CH * st;
        if (e0 + 8 * CH <= d) {
#pragma unroll
            for (uint32_t i = 0; i < CH; i++) s = f16_piece_fold(w[i].x, w[i].y, w[i].z, w[i].w, yq + e0 + 8 * i, s);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < CH; i++) {
                const uint32_t e = e0 + 8 * i;
                if (e >= d) continue;
                if (e + 8 <= d)
                    s = f16_piece_fold(w[i].x, w[i].y, w[i].z, w[i].w, yq + e, s);
                else
                    s = f16_piece_fold_tail(w[i].x, w[i].y, w[i].z, w[i].w, yq + e, d - e, s);
            }
        }
        return s;
    };
    float s = 0.0f;
    fetch(a, 0);
#pragma unroll 1
    for (uint32_t st = 0; st < nst; st += 2) {
        if (st + 1 < nst) fetch(b, st + 1);
        s = fold(a, st, s);
        if (st + 2 < nst) fetch(a, st + 2);
        if (st + 1 < nst) s = fold(b, st + 1, s);
    }
    return s;
}

// ---------------------------------------------------------------------------------------------
// Rows of whole 128-byte lines (d a multiple of 64), gathered COOPERATIVELY -- the f16 form of coop_rows.inc, for the
// reason stated there: a lane per row asks for every line with eight instructions of 16 bytes each, and that request
// shape tops out far below HBM's rate on a table beyond the caches.
//
// The wave's wanted rows are ranked (rank = wanted lanes below, mbcnt of the ballot).  A load instruction covers stage s
// of 64 / LPR rows: lane (g, t) = (lane / LPR, lane % LPR) reads bytes [16 t, 16 t + 16) of the stage for the row of rank
// (64 / LPR) i + g.  LPR = 8: a stage is a whole line (64 elements) and four instructions serve 32 rows; LPR = 4: half a
// line (32 elements), four instructions serve 64 rows -- taken when more than 32 rows are wanted (a candidate's fresh
// neighbours plus the runner-up's), so that one round still serves every row.  K stages are in flight in registers.  A
// landed stage goes through a 4-KiB LDS image, its 16-byte pieces XOR-swizzled so that the owner lane's read of its own
// row's stage -- LPR ds_read_b128 -- is conflict-free; the owner widens the pieces and continues its own chain.
//
// Stage depth K = 4: 4 stages x 4 loads x 16 B x 64 lanes = 16 KiB in flight per wave, the bytes in flight at which the f32
// gather measured best (profiles/r03_config2_coop_stage_depth.txt: K = 8 no faster, 12 slower for want of registers);
// a stage here carries twice the elements, so d = 128 and 256 have the whole row in flight and d = 768 a third of it.
// Chosen by that reasoning, not measured again for f16.
//
// ids_s: 64 words of LDS (rank -> row id); img: the 4-KiB stage image, 16-byte aligned.  Returns the lane's sum (0 for a
// lane that wants nothing); all 64 lanes call it together.
// ---------------------------------------------------------------------------------------------
constexpr int HX_R16_K = 4;
template <int DS>
__host__ __device__ constexpr bool coop_rows16() {
    return DS >= 128 && DS % 64 == 0;
}

template <int DS, int LPR>
__device__ __forceinline__ float f16_rows_coop_round(const uint8_t *rows, bool mine, uint32_t rank, uint32_t nw,
                                                     const float *yq, const uint32_t *ids_s, unsigned char *img, int lane) {
    constexpr int SB = 16 * LPR;         // bytes of a row per stage
    constexpr int EPS = SB / 2;          // elements of a row per stage
    constexpr int RPI = 64 / LPR;        // rows per load instruction
    constexpr int NS = DS * 2 / SB;      // stages per row
    constexpr int KK = HX_R16_K < NS ? HX_R16_K : NS;
    static_assert(NS % KK == 0, "the stage ring divides the row");
    constexpr size_t ROWB = (size_t)DS * 2;
    constexpr uint32_t SWS = LPR == 8 ? 1 : 2, SWM = LPR - 1;
    const uint32_t g = (uint32_t)lane / LPR, t = (uint32_t)lane % LPR;
    // rows of instruction i: rank RPI i + g; a rank past the end repeats the last row (the same line again: no exec
    // masks in the stream, no new traffic)
    const uint8_t *src[4];
    uint32_t wofs[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t slot = (uint32_t)RPI * i + g;
        const uint32_t rr = min(slot, nw - 1);
        src[i] = rows + (size_t)ids_s[rr] * ROWB + 16u * t;
        wofs[i] = slot * SB + ((t ^ ((slot >> SWS) & SWM)) << 4);
    }
    const unsigned char *rd = img + rank * SB;
    const uint32_t sw = (rank >> SWS) & SWM;
    u32x4 w[KK][4];
    float s = 0.0f;
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
#pragma unroll
            for (int k = 0; k < LPR; k++) {
                const uint4 pp = *reinterpret_cast<const uint4 *>(rd + (((uint32_t)k ^ sw) << 4));
                s = f16_piece_fold(pp.x, pp.y, pp.z, pp.w, yq + EPS * st + 8 * k, s);
            }
        }
        // the next stage's image may only be written once every owner has read this one: one wave's LDS operations
        // execute in issue order, the clobber keeps the compiler from moving them across
        asm volatile("" ::: "memory");
    };
#pragma unroll
    for (int j = 0; j < KK; j++) request(j, j);
#pragma unroll 1
    for (int st0 = 0; st0 + KK < NS; st0 += KK) {  // every slot is refilled
#pragma unroll
        for (int j = 0; j < KK; j++) {
            to_image(j);
            request(j, st0 + KK + j);
            owners_sum(st0 + j);
        }
    }
#pragma unroll
    for (int j = 0; j < KK; j++) {  // the last KK stages
        to_image(j);
        owners_sum(NS - KK + j);
    }
    return s;
}

template <int DS>
__device__ __forceinline__ float f16_rows_coop(const uint8_t *rows, uint32_t id, bool active, const float *yq,
                                               uint32_t *ids_s, unsigned char *img, int lane) {
    static_assert(DS % 64 == 0, "whole 128-byte lines");
    const u64 W = __ballot(active);
    const uint32_t nw = (uint32_t)__popcll(W);
    if (nw == 0) return 0.0f;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(W >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)W, 0u));
    if (active) ids_s[rank] = id;
    wave_fence();
    if (nw <= 32) return f16_rows_coop_round<DS, 8>(rows, active, rank, nw, yq, ids_s, img, lane);
    return f16_rows_coop_round<DS, 4>(rows, active, rank, nw, yq, ids_s, img, lane);
}
