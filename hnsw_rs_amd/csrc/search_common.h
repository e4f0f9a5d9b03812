// search_common.h -- the device primitives that more than one .hip uses (search_kernels.hip, search_lean.hip,
// build_kernels.hip, exact_scan.hip, search_filtered.hip).  gfx950 only; include from .hip files.
//   lanes        readlane64, pair_swap*, wave_fence
//   quantiser    f32_as_u8, stage_query (a query), stage_row (a stored point as the query), QLds / QRegs
//   distances    quant_half_sums (QuantVec::distance_unrolled, two lanes per row),
//                quant_bulk_stages, dist_any_dim (any dimension), f32_row_sum / f32_row_sum_staged (compile-time
//                dimension), coop_rows.inc (the cooperative whole-line gather, included below), dist_build
//   memory       dma_piece_to_lds (global -> LDS without a register), asm_ld32 / asm_ld128
//   the list     KEY_*, HX_MAX_R, HX_MAX_R_WIDE, WaveList, merge_prefix
//   visited set  visited_contains, visited_insert (the LDS table)
// The cycle-stamp macros stay with the kernels that carry stamps (search_kernels.hip, search_lean.hip).
#pragma once

#include "device_index.h"

namespace hx {

typedef unsigned long long u64;
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u64 readlane64(u64 v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((u64)hi << 32) | lo;
}
// value held by the other lane of this lane's pair (lane ^ 1): DPP quad_perm [1,0,3,2]
__device__ __forceinline__ float pair_swap(float x) {
    return __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, true));
}
__device__ __forceinline__ int pair_swap_i(int x) {
    return __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true);
}
// Orders this wave's LDS traffic (one wave's DS operations execute in issue order; the clobber keeps
// the compiler from moving accesses across).  The per-query state of a wave is private to it, so no
// workgroup barrier is needed -- and none may be used where only some waves of a workgroup run.
__device__ __forceinline__ void wave_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// Rust `f32 as u8`: saturating, NaN -> 0
__device__ __forceinline__ uint32_t f32_as_u8(float x) {
    if (!(x > 0.0f)) return 0;
    if (x >= 255.0f) return 255;
    return (uint32_t)x;
}

// ---------------------------------------------------------------------------------------------
// distance of this lane's share of one QUANT8 row (quant.rs:14-37).
// P 16-byte pieces per half row; element e of the half sits at byte 8 + e.  Elements below nch4
// are chunk elements (running sum e & 3 of this lane), elements [nch4, nch4 + rem) are the tail
// and all go to running sum 0 of lane h == 0, in order, after its chunk elements.
// yq: this half's dequantised query values in the same element order (LDS or registers).
// ---------------------------------------------------------------------------------------------
template <int P, int DS, typename QSrc>
__device__ __forceinline__ void quant_half_sums(const uint4 (&w)[P], const QSrc &yq, int h,
                                                uint32_t nch4, uint32_t rem, float (&acc)[4]) {
    const float mn = __builtin_bit_cast(float, w[0].x);
    const float delta = __builtin_bit_cast(float, w[0].y);
#pragma unroll
    for (int p = 0; p < P; p++) {
        const uint32_t dw[4] = {w[p].x, w[p].y, w[p].z, w[p].w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (p == 0 && j < 2) continue;  // header
            if (DS > 0) {
                // compile-time dimension: dead elements vanish; the four bytes of a chunk dword feed
                // running sums 0..3 as two packed pairs (v_pk_mul_f32 / v_pk_add_f32: per element the
                // same correctly rounded operations as the scalar form)
                constexpr int N4 = 4 * (DS / 8);
                const int e0 = 16 * p + 4 * j - 8;
                if (e0 + 3 < N4) {
#pragma unroll
                    for (int k = 0; k < 4; k += 2) {
                        const f32x2 c = {(float)((dw[j] >> (8 * k)) & 0xFFu),
                                         (float)((dw[j] >> (8 * (k + 1))) & 0xFFu)};
                        const f32x2 x = c * delta + mn;
                        const f32x2 y = {yq[e0 + k], yq[e0 + k + 1]};
                        const f32x2 t = x - y;
                        const f32x2 t2 = t * t;
                        acc[k] += t2.x;
                        acc[k + 1] += t2.y;
                    }
                    continue;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int e = 16 * p + 4 * j + k - 8;
                if (DS > 0) {  // the tail of a compile-time dimension
                    constexpr int N4 = 4 * (DS / 8), RM = DS % 8;
                    if (e >= N4 + RM) continue;
                    const float x = ((float)((dw[j] >> (8 * k)) & 0xFFu) * delta) + mn;
                    const float t = x - yq[e];
                    const float t2 = t * t;
                    if (e < N4)
                        acc[k] += t2;
                    else
                        acc[0] += (h == 0) ? t2 : 0.0f;  // +0.0 leaves a non-negative sum as is
                } else {
                    const float x = ((float)((dw[j] >> (8 * k)) & 0xFFu) * delta) + mn;
                    const float t = x - yq[e];
                    const float t2 = t * t;
                    const bool chunk = (uint32_t)e < nch4;
                    const bool tail = !chunk && (uint32_t)e < nch4 + rem && h == 0;
                    if (k == 0) {
                        acc[0] += (chunk || tail) ? t2 : 0.0f;
                    } else {
                        acc[k] += chunk ? t2 : 0.0f;
                        acc[0] += tail ? t2 : 0.0f;
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Stage one query in LDS.  QUANT8: the query is quantised with its own min / delta exactly like
// a stored vector (Point::new -> QuantVec::new, template.rs:313, quant.rs:41-66) and kept
// dequantised, y = code * delta + min, split into the two half-row element orders:
// yq[h * nq_half + i].  F32: the raw values.  Returns false when the query holds a NaN
// (partial_cmp().unwrap() panics in the reference).
// ---------------------------------------------------------------------------------------------
template <int KIND>
__device__ __forceinline__ bool stage_query(const DevView &v, const float *qv, float *yq, int lane) {
    const uint32_t d = v.dim;
    bool bad = false;
    if (KIND == HNSW_VEC_QUANT8) {
        const uint32_t nq_half = v.half_bytes - 8;
        float lo = __builtin_inff(), hi = -__builtin_inff();
        for (uint32_t e = lane; e < d; e += 64) {
            const float x = qv[e];
            bad |= (x != x);
            lo = fminf(lo, x);
            hi = fmaxf(hi, x);
        }
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o));
            hi = fmaxf(hi, __shfl_xor(hi, o));
        }
        const float delta = (hi - lo) / 255.0f;  // (ub - lb) / (2^8 - 1)
        for (uint32_t e = lane; e < 2 * nq_half; e += 64) yq[e] = 0.0f;
        wave_fence();
        const uint32_t full = d & ~7u;
        for (uint32_t e = lane; e < d; e += 64) {
            float b = (qv[e] - lo) / delta;
            b += 0.5f;
            const float y = ((float)f32_as_u8(floorf(b)) * delta) + lo;
            uint32_t hh, i;
            if (e < full) {
                hh = (e & 7) >> 2;
                i = 4 * (e >> 3) + (e & 3);
            } else {
                hh = 0;
                i = v.nch4 + (e - full);
            }
            yq[hh * nq_half + i] = y;
        }
    } else {
        for (uint32_t e = lane; e < d; e += 64) {
            const float x = qv[e];
            bad |= (x != x);
            yq[e] = x;
        }
    }
    wave_fence();
    return __ballot(bad) == 0;
}

// LDS-resident query values of one half
struct QLds {
    const float *p;
    __device__ __forceinline__ float operator[](int e) const { return p[e]; }
};
// register-resident query values (compile-time dimension)
template <int N>
struct QRegs {
    float v[N];
    __device__ __forceinline__ float operator[](int e) const { return v[e]; }
};

static constexpr u64 KEY_INVALID = ~0ull;
static constexpr u64 KEY_MASK = 0x7FFFFFFFFFFFFFFFull;  // drops the expanded flag
static constexpr u64 KEY_EXPANDED = 1ull << 63;

#define HX_MAX_R 8  // ef <= 64 * HX_MAX_R on the specialised kernels and in the on-device build
#define HX_MAX_R_WIDE 16  // ef <= 1024 on the any-dimension search kernel

// ---------------------------------------------------------------------------------------------
// Stage a STORED point as the query (build path: Point::dist2other between two stored points,
// points/src/points.rs:86-93).  QUANT8: the packed row already is in the half-row element order, so
// yq[h * nq_half + e] = code * delta + min straight from the row.  F32: the row's floats.
// ---------------------------------------------------------------------------------------------
template <int KIND>
__device__ __forceinline__ void stage_row(const DevView &v, uint32_t id, float *yq, int lane) {
    if (KIND == HNSW_VEC_QUANT8) {
        const uint32_t nq_half = v.half_bytes - 8;
        const uint8_t *row = v.rows + (size_t)id * v.row_stride;
        for (uint32_t i = lane; i < 2 * nq_half; i += 64) {
            const uint32_t hh = i >= nq_half ? 1u : 0u, e = i - hh * nq_half;
            const uint8_t *half = row + hh * v.half_bytes;
            const float mn = *reinterpret_cast<const float *>(half);
            const float delta = *reinterpret_cast<const float *>(half + 4);
            const bool used = e < v.nch4 || (hh == 0 && e < v.nch4 + v.rem);
            yq[i] = used ? ((float)half[8 + e] * delta) + mn : 0.0f;
        }
    } else {
        const float *row = reinterpret_cast<const float *>(v.rows + (size_t)id * v.row_stride);
        for (uint32_t e = lane; e < v.dim; e += 64) yq[e] = row[e];
    }
    wave_fence();
}

// ---------------------------------------------------------------------------------------------
// QUANT8, any dimension: the pieces of a half row that hold nothing but chunk elements, without
// per-element predicates, in stages of CH 16-byte pieces through two register buffers (the next
// stage in flight while the current one is summed).  Starts at piece `first` >= 1 (piece 0 carries the
// header); returns the number of pieces consumed (a multiple of CH).  Element e of the half sits at
// byte 8 + e.
// ---------------------------------------------------------------------------------------------
template <int CH>
__device__ __forceinline__ uint32_t quant_bulk_stages(const uint4 *src, const float *yh, float delta, float mn,
                                                      uint32_t first, uint32_t n_pure, float (&acc)[4]) {
    const uint32_t nst = n_pure / CH;
    if (nst == 0) return 0;
    uint4 a[CH], b[CH];
    auto fetch_at = [&](uint4 (&w)[CH], uint32_t st) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < CH; i++) w[i] = src[first + st * CH + i];
    };
    auto consume_at = [&](const uint4 (&w)[CH], uint32_t st) __attribute__((always_inline)) {
        const float *y = yh + 16 * (first + st * CH) - 8;  // query value of the stage's first element
#pragma unroll
        for (int i = 0; i < CH; i++) {
            const uint32_t dw[4] = {w[i].x, w[i].y, w[i].z, w[i].w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
#pragma unroll
                for (int k = 0; k < 4; k += 2) {
                    const f32x2 c = {(float)((dw[j] >> (8 * k)) & 0xFFu), (float)((dw[j] >> (8 * (k + 1))) & 0xFFu)};
                    const f32x2 x = c * delta + mn;
                    const f32x2 yy = {y[16 * i + 4 * j + k], y[16 * i + 4 * j + k + 1]};
                    const f32x2 t = x - yy;
                    const f32x2 t2 = t * t;
                    acc[k] += t2.x;
                    acc[k + 1] += t2.y;
                }
            }
        }
    };
    fetch_at(a, 0);
#pragma unroll 1
    for (uint32_t st = 0; st < nst; st += 2) {
        if (st + 1 < nst) fetch_at(b, st + 1);
        consume_at(a, st);
        if (st + 2 < nst) fetch_at(a, st + 2);
        if (st + 1 < nst) consume_at(b, st + 1);
    }
    return nst * CH;
}

// ---------------------------------------------------------------------------------------------
// Distance of one stored point to the staged query for ANY dimension (runtime loops): used by
// the test-seam and brute-force kernels, and by the search kernel when no specialised variant
// fits.  QUANT8: valid on the even lane of the pair; F32: per lane.
// ---------------------------------------------------------------------------------------------
template <int KIND>
__device__ __forceinline__ float dist_any_dim(const DevView &v, uint32_t id, bool active, int h,
                                              const float *yq) {
    if (KIND == HNSW_VEC_QUANT8) {
        const float *yh = yq + h * (v.half_bytes - 8);
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (active) {
            const uint4 *src = reinterpret_cast<const uint4 *>(
                v.rows + (size_t)id * v.row_stride + (size_t)h * v.half_bytes);
            const uint32_t np = v.half_bytes >> 4;
            const uint4 w0 = src[0];
            const float mn = __builtin_bit_cast(float, w0.x);
            const float delta = __builtin_bit_cast(float, w0.y);
            // Pieces [p_lo, p_hi) through the predicated element loop, 4 pieces (64 B) per group.
            auto consume_pred = [&](uint32_t p_lo, uint32_t p_hi) __attribute__((always_inline)) {
                for (uint32_t p0 = p_lo; p0 < p_hi; p0 += 4) {
                    uint4 w[4];
#pragma unroll
                    for (int p = 0; p < 4; p++)
                        w[p] = (p0 + p < p_hi) ? src[p0 + p] : make_uint4(0, 0, 0, 0);
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        if (p0 + p >= p_hi) continue;  // wave-uniform: a piece outside the range costs nothing
                        const uint32_t dw[4] = {w[p].x, w[p].y, w[p].z, w[p].w};
#pragma unroll
                        for (int j = 0; j < 4; j++) {
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                const int e = 16 * (int)(p0 + p) + 4 * j + k - 8;
                                const float x = ((float)((dw[j] >> (8 * k)) & 0xFFu) * delta) + mn;
                                const bool chunk = e >= 0 && (uint32_t)e < v.nch4;
                                const bool tail = e >= 0 && !chunk &&
                                                  (uint32_t)e < v.nch4 + v.rem && h == 0;
                                const float y = (chunk || tail) ? yh[e] : 0.0f;
                                const float t = x - y;
                                const float t2 = t * t;
                                if (k == 0) {
                                    acc[0] += (chunk || tail) ? t2 : 0.0f;
                                } else {
                                    acc[k] += chunk ? t2 : 0.0f;
                                    acc[0] += tail ? t2 : 0.0f;
                                }
                            }
                        }
                    }
                }
            };
            // Pieces 1 .. that hold nothing but chunk elements go through the predicate-free stages
            // (quant_bulk_stages); piece 0 (header) before, the remainder after -- every running sum
            // still sees its elements in ascending order.
            const uint32_t n_pure = v.nch4 >= 24 ? (v.nch4 - 8) / 16 : 0;  // pieces [1, 1 + n_pure)
            if (n_pure < 4) {
                consume_pred(0, np);
            } else {
                consume_pred(0, 1);
                // widest stages first, then narrower ones over what is left of the pure pieces
                uint32_t used = 0;
                if (n_pure >= 16) used += quant_bulk_stages<8>(src, yh, delta, mn, 1, n_pure, acc);
                used += quant_bulk_stages<4>(src, yh, delta, mn, 1 + used, n_pure - used, acc);
                used += quant_bulk_stages<1>(src, yh, delta, mn, 1 + used, n_pure - used, acc);
                consume_pred(1 + used, np);
            }
        }
        // acc.iter().sum(): ((((((a0+a1)+a2)+a3)+a4)+a5)+a6)+a7 with a4..a7 on the odd lane
        const float b0 = pair_swap(acc[0]), b1 = pair_swap(acc[1]), b2 = pair_swap(acc[2]),
                    b3 = pair_swap(acc[3]);
        float s = 0.0f;
        s += acc[0];
        s += acc[1];
        s += acc[2];
        s += acc[3];
        s += b0;
        s += b1;
        s += b2;
        s += b3;
        return __builtin_sqrtf(s);
    } else {
        // FullVec: one sequential sum per candidate, one candidate per lane (full.rs:24-28)
        float s = 0.0f;
        if (active) {
            const uint4 *src = reinterpret_cast<const uint4 *>(v.rows + (size_t)id * v.row_stride);
            const uint32_t np = v.row_stride >> 4, d = v.dim;
            // bulk: whole pairs of 16-piece stages, two register buffers, the next stage in flight
            // while the current one is summed (one exposed round trip per 512 B instead of per 128 B);
            // only pieces that lie entirely inside the row's d floats take this path
            constexpr uint32_t CH = 16;
            const uint32_t full_pieces = d >> 2;                      // pieces without padding floats
            const uint32_t pairs = full_pieces / (2 * CH);
            uint32_t p_done = 0;
            if (pairs > 0) {
                uint4 a[CH], b[CH];
                auto fetch_at = [&](uint4 (&w)[CH], const uint4 *p) __attribute__((always_inline)) {
#pragma unroll
                    for (uint32_t i = 0; i < CH; i++) w[i] = p[i];
                };
                auto consume_at = [&](const uint4 (&w)[CH], const float *y) __attribute__((always_inline)) {
#pragma unroll
                    for (uint32_t i = 0; i < CH; i++) {
                        const uint32_t dw[4] = {w[i].x, w[i].y, w[i].z, w[i].w};
#pragma unroll
                        for (int j = 0; j < 4; j += 2) {
                            const f32x2 x = {__builtin_bit_cast(float, dw[j]), __builtin_bit_cast(float, dw[j + 1])};
                            const f32x2 yy = {y[4 * i + j], y[4 * i + j + 1]};
                            const f32x2 t = x - yy;
                            const f32x2 t2 = t * t;
                            s += t2.x;
                            s += t2.y;
                        }
                    }
                };
                fetch_at(a, src);
#pragma unroll 1
                for (uint32_t pr = 0; pr < pairs; pr++) {
                    const uint32_t st = 2 * pr;
                    fetch_at(b, src + (st + 1) * CH);
                    consume_at(a, yq + 4 * st * CH);
                    if (pr + 1 < pairs) fetch_at(a, src + (st + 2) * CH);
                    consume_at(b, yq + 4 * (st + 1) * CH);
                }
                p_done = pairs * 2 * CH;
            }
            for (uint32_t p0 = p_done; p0 < np; p0 += 8) {
                uint4 w[8];
#pragma unroll
                for (int p = 0; p < 8; p++)
                    w[p] = (p0 + p < np) ? src[p0 + p] : make_uint4(0, 0, 0, 0);
#pragma unroll
                for (int p = 0; p < 8; p++) {
                    const uint32_t dw[4] = {w[p].x, w[p].y, w[p].z, w[p].w};
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const uint32_t e = 4 * (p0 + p) + j;
                        const bool in = e < d;
                        const float y = in ? yq[e] : 0.0f;
                        const float t = __builtin_bit_cast(float, dw[j]) - y;
                        const float t2 = t * t;
                        s += in ? t2 : 0.0f;  // +0.0 leaves a non-negative sum unchanged
                    }
                }
            }
        }
        return __builtin_sqrtf(s);
    }
}

// Asynchronous global -> LDS copy of one 1-KiB piece (64 lanes x 16 bytes): lane l's 16 bytes at
// `gsrc` land at LDS byte address lds_dst + 16 l.  No VGPR destination, and -- being inline asm --
// not part of the compiler's s_waitcnt bookkeeping, so the copy stays in flight across the loops
// and LDS atomics of the expansion body (hipcc drains vmcnt(0) at every loop it cannot see
// through).  The consumer issues its own `s_waitcnt vmcnt(0)` before reading the bytes back
// (cdna_hip_programming.md section 5.7: M0 is written in the same statement that reads it).
__device__ __forceinline__ void dma_piece_to_lds(const void *gsrc, uint32_t lds_dst) {
    lds_dst = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_dst);  // provably wave-uniform
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gsrc), "s"(lds_dst)
        : "memory");
}

// Loads that the compiler's s_waitcnt bookkeeping does not see, each with its own wait.  They serve
// the rare degree > 32 rows inside the inline-rows loops: a single compiler-visible VMEM load
// anywhere in that loop nest makes hipcc drain vmcnt(0) at the loop header on EVERY iteration,
// which would serialise the block prefetch (measured: the prefetch then gains nothing).
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t asm_ld32(const void *p) {
    uint32_t r;
    asm volatile("global_load_dword %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=&v"(r) : "v"(p) : "memory");
    return r;
}
__device__ __forceinline__ uint4 asm_ld128(const void *p) {
    u32x4 r;
    asm volatile("global_load_dwordx4 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=&v"(r) : "v"(p) : "memory");
    return make_uint4(r.x, r.y, r.z, r.w);
}

// FullVec row against the staged query when the dimension is a compile-time constant: all P
// 16-byte pieces of the row are loaded up front (P x 16 bytes in flight per lane), the sum is the
// reference's single left-to-right chain (full.rs:24-28).
template <int P, int DS>
__device__ __forceinline__ float f32_row_sum(const uint4 (&w)[P], const float *yq) {
    // x - y and the square run two elements per instruction (v_pk_add_f32 / v_pk_mul_f32: each
    // element is the same correctly rounded IEEE operation); the sum stays the one serial chain
    float s = 0.0f;
#pragma unroll
    for (int p = 0; p < P; p++) {
        const uint32_t dw[4] = {w[p].x, w[p].y, w[p].z, w[p].w};
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
            const int e = 4 * p + j;
            if (e >= DS) continue;
            if (e + 1 < DS) {
                const f32x2 x = {__builtin_bit_cast(float, dw[j]), __builtin_bit_cast(float, dw[j + 1])};
                const f32x2 y = {yq[e], yq[e + 1]};
                const f32x2 t = x - y;
                const f32x2 t2 = t * t;
                s += t2.x;
                s += t2.y;
            } else {
                const float t = __builtin_bit_cast(float, dw[j]) - yq[e];
                s += t * t;
            }
        }
    }
    return s;
}

// Wide f32 rows (d > 192): the same single chain, with the row streamed through two register buffers
// of CH 16-byte pieces each.  The stage loop has a compile-time trip count and is fully unrolled, so
// the code is straight-line: the loads of stage s + 1 are in flight while stage s is summed and the
// compiler's s_waitcnt counts are exact (a rolled loop drains them at its header).
#ifndef HX_WIDE_CH
#define HX_WIDE_CH 16  // 16-byte pieces per stage buffer of the wide-row loop (two buffers in flight per lane)
#endif
template <int DS, int CH, bool ROLLED>
__device__ __forceinline__ float f32_row_sum_staged(const uint4 *src, const float *yq) {
    constexpr int NP = (DS + 3) / 4, NST = (NP + CH - 1) / CH;
    static_assert(!ROLLED || (NP % (2 * CH) == 0), "the rolled form needs whole stage pairs");
    uint4 a[CH], b[CH];
    float s = 0.0f;
    auto fetch = [&](uint4 (&w)[CH], int st) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < CH; p++)
            if (st * CH + p < NP) w[p] = src[st * CH + p];
    };
    auto consume = [&](const uint4 (&w)[CH], int st) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < CH; p++) {
            if (st * CH + p >= NP) continue;
            const uint32_t dw[4] = {w[p].x, w[p].y, w[p].z, w[p].w};
#pragma unroll
            for (int j = 0; j < 4; j += 2) {
                const int e = 4 * (st * CH + p) + j;
                if (e >= DS) continue;
                if (e + 1 < DS) {
                    const f32x2 x = {__builtin_bit_cast(float, dw[j]), __builtin_bit_cast(float, dw[j + 1])};
                    const f32x2 y = {yq[e], yq[e + 1]};
                    const f32x2 t = x - y;
                    const f32x2 t2 = t * t;
                    s += t2.x;
                    s += t2.y;
                } else {
                    const float t = __builtin_bit_cast(float, dw[j]) - yq[e];
                    s += t * t;
                }
            }
        }
    };
    if constexpr (ROLLED) {
        // very wide rows: the unrolled form outgrows the instruction cache (d = 768: 3.9 ms against
        // 1.9 ms for the plain loop), so the stage pairs stay a loop -- one exposed round trip per
        // 2 CH pieces instead of one per 8
        auto fetch_at = [&](uint4 (&w)[CH], const uint4 *p) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < CH; i++) w[i] = p[i];
        };
        auto consume_at = [&](const uint4 (&w)[CH], const float *y) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < CH; i++) {
                const uint32_t dw[4] = {w[i].x, w[i].y, w[i].z, w[i].w};
#pragma unroll
                for (int j = 0; j < 4; j += 2) {
                    const f32x2 x = {__builtin_bit_cast(float, dw[j]), __builtin_bit_cast(float, dw[j + 1])};
                    const f32x2 yy = {y[4 * i + j], y[4 * i + j + 1]};
                    const f32x2 t = x - yy;
                    const f32x2 t2 = t * t;
                    s += t2.x;
                    s += t2.y;
                }
            }
        };
        static_assert(DS % 4 == 0, "whole pieces");
        fetch_at(a, src);
#pragma unroll 1
        for (int st = 0; st < NST; st += 2) {
            fetch_at(b, src + (st + 1) * CH);
            consume_at(a, yq + 4 * st * CH);
            if (st + 2 < NST) fetch_at(a, src + (st + 2) * CH);
            consume_at(b, yq + 4 * (st + 1) * CH);
        }
        return s;
    }
    fetch(a, 0);
#pragma unroll
    for (int st = 0; st < NST; st += 2) {
        if (st + 1 < NST) fetch(b, st + 1);
        consume(a, st);
        if (st + 2 < NST) fetch(a, st + 2);
        if (st + 1 < NST) consume(b, st + 1);
    }
    return s;
}

#include "coop_rows.inc"

// ---------------------------------------------------------------------------------------------
// Distance of a stored point to the staged row on the build path.  DS > 0: the dimension is a
// compile-time constant (all row pieces in flight, dead elements vanish), otherwise the runtime
// loops of dist_any_dim.  QUANT8: valid on the even lane of the pair; F32: per lane.
// ---------------------------------------------------------------------------------------------
// COOP (insert kernel, f32 rows of whole lines): the cooperative gather of coop_rows.inc through ids_s
// (64 words) and img (4 KiB) -- the insertion searches of a 50-100M point build read rows scattered over
// tens of GB, where the lane-per-row shape tops out at 1.2 TB/s (profiles/r03_gather_shapes_*.txt).
template <int KIND, int DS, bool COOP = false>
__device__ __forceinline__ float dist_build(const DevView &v, uint32_t id, bool active, int h, const float *yq,
                                            uint32_t *ids_s = nullptr, unsigned char *img = nullptr, int lane = 0) {
    if constexpr (COOP && coop_rows<KIND, DS>()) {
        return __builtin_sqrtf(f32_rows_coop<(DS > 0 ? DS : 32), HX_COOP_K>(v.rows, id, active, yq, ids_s, img, lane));
    } else if constexpr (DS > 0 && KIND == HNSW_VEC_QUANT8) {
        constexpr int NQ = 4 * (DS / 8) + DS % 8;  // elements of half 0 (half 1 has DS % 8 fewer)
        constexpr int P = (8 + NQ + 15) / 16;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (active) {
            const uint4 *src = reinterpret_cast<const uint4 *>(
                v.rows + (size_t)id * v.row_stride + (size_t)h * v.half_bytes);
            uint4 w[P];
#pragma unroll
            for (int p = 0; p < P; p++) w[p] = src[p];
            __builtin_amdgcn_sched_barrier(0);  // every piece requested before the arithmetic
            const QLds q{yq + h * (v.half_bytes - 8)};
            quant_half_sums<P, DS>(w, q, h, v.nch4, v.rem, acc);
        }
        const float b0 = pair_swap(acc[0]), b1 = pair_swap(acc[1]), b2 = pair_swap(acc[2]),
                    b3 = pair_swap(acc[3]);
        float s = 0.0f;
        s += acc[0];
        s += acc[1];
        s += acc[2];
        s += acc[3];
        s += b0;
        s += b1;
        s += b2;
        s += b3;
        return __builtin_sqrtf(s);
    } else if constexpr (DS > 0 && KIND == HNSW_VEC_F32) {
        constexpr int P = (DS + 3) / 4;
        float sm = 0.0f;
        if (active) {
            const uint4 *src = reinterpret_cast<const uint4 *>(v.rows + (size_t)id * v.row_stride);
            uint4 w[P];
#pragma unroll
            for (int p = 0; p < P; p++) w[p] = src[p];
            __builtin_amdgcn_sched_barrier(0);
            sm = f32_row_sum<P, DS>(w, yq);
        }
        return __builtin_sqrtf(sm);
    } else {
        return dist_any_dim<KIND>(v, id, active, h, yq);
    }
}

// ---------------------------------------------------------------------------------------------
// Per-wave search state and the pieces of search_layer
// ---------------------------------------------------------------------------------------------
template <int R>
struct WaveList {
    u64 L[R];         // list[64 r + lane]; KEY_INVALID beyond n_cur
    uint32_t n_cur;   // wave-uniform
    u64 last_key;     // key (flag dropped) of position ef - 1 when the list is full

    // Merge the wave's candidate keys (KEY_INVALID = none) into the sorted list, keeping the ef
    // smallest: streaming top-ef of searcher.rs:74-94 for a whole batch (order-independent).
    // new_flag (0 or KEY_EXPANDED) is OR-ed into every key that enters the list
    __device__ __forceinline__ void merge(u64 key, uint32_t ef, u64 *perm, int lane, u64 new_flag = 0) {
        const bool full = n_cur >= ef;
        const bool surv = key != KEY_INVALID && (!full || key < last_key);
        u64 smask = __ballot(surv);
        if (smask == 0) return;
        const uint32_t m = (uint32_t)__popcll(smask);
        if (m <= (R == 1 ? 4u : 0u)) {
            // few survivors (the usual case once the list is full): insert them one at a time by
            // shifting the tail of the register-resident list one lane to the right (DPP
            // wave_shr:1, no LDS round trip).  Insertion order is irrelevant (N2).  Only for one-
            // register lists: with R > 1 every insert shifts R registers with a carry, and the
            // rank-scatter below is cheaper even for a single survivor (f32 efSearch 68: 0.266 ->
            // 0.255 ms; SQ counters had shown +33 % VALU instructions per query for R = 2 vs R = 1).
            u64 it = smask;
            while (it) {
                const int j = __ffsll((long long)it) - 1;
                it &= it - 1;
                const u64 e = readlane64(key, j);
                if (n_cur >= ef && !(e < last_key)) continue;  // an earlier insert tightened the bound
                uint32_t pos = 0;
#pragma unroll
                for (int r = 0; r < R; r++)
                    pos += (uint32_t)__popcll(__ballot((L[r] & KEY_MASK) < e));
                u64 carry = 0;  // lane 63 of the previous register feeds lane 0 of the next
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const uint32_t idx = 64u * r + lane;
                    const uint32_t lo = (uint32_t)L[r], hi = (uint32_t)(L[r] >> 32);
                    uint32_t slo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, 0x138, 0xF, 0xF, false);
                    uint32_t shi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, 0x138, 0xF, 0xF, false);
                    u64 sh = ((u64)shi << 32) | slo;
                    if (lane == 0) sh = carry;
                    if (R > 1) carry = readlane64(L[r], 63);
                    if (idx == pos)
                        L[r] = e | new_flag;
                    else if (idx > pos)
                        L[r] = sh;
                }
                n_cur = min(n_cur + 1, ef);
#pragma unroll
                for (int r = 0; r < R; r++)
                    if (64u * r + lane >= n_cur) L[r] = KEY_INVALID;
                refresh_last(ef);
            }
            return;
        }
        uint32_t shift[R];
#pragma unroll
        for (int r = 0; r < R; r++) shift[r] = 0;
        uint32_t my_rank = 0;
        u64 it = smask;
        while (it) {  // wave-uniform loop over the survivors
            const int j = __ffsll((long long)it) - 1;
            it &= it - 1;
            const u64 e = readlane64(key, j);
            uint32_t below = 0;  // list entries smaller than e
#pragma unroll
            for (int r = 0; r < R; r++) {
                const bool lt = (L[r] & KEY_MASK) < e;  // invalid entries are the maximum
                below += (uint32_t)__popcll(__ballot(lt));
                shift[r] += lt ? 0u : 1u;
            }
            if (surv && e < key) my_rank++;
            if (lane == j) my_rank += below;
        }
        // scatter to the new positions through LDS (all reads of L happened above)
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t idx = 64u * r + lane;
            const uint32_t np = idx + shift[r];
            if (idx < n_cur && np < ef) perm[np] = L[r];
        }
        if (surv && my_rank < ef) perm[my_rank] = key | new_flag;
        n_cur = min(n_cur + m, ef);
        wave_fence();  // single-wave workgroup: orders the LDS writes before the reads
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t idx = 64u * r + lane;
            L[r] = idx < n_cur ? perm[idx] : KEY_INVALID;
        }
        wave_fence();
        refresh_last(ef);
    }

    __device__ __forceinline__ void refresh_last(uint32_t ef) {
        if (n_cur >= ef) {
            const uint32_t pos = ef - 1;
            u64 k = 0;
#pragma unroll
            for (int r = 0; r < R; r++)
                if ((pos >> 6) == (uint32_t)r) k = readlane64(L[r], pos & 63);
            last_key = k & KEY_MASK;
        } else {
            last_key = KEY_INVALID;
        }
    }

    // position of the smallest entry not expanded yet, -1 if none (the loop of searcher.rs:35)
    __device__ __forceinline__ int first_unexpanded(int lane) const {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t idx = 64u * r + lane;
            const u64 mk = __ballot(idx < n_cur && (L[r] & KEY_EXPANDED) == 0);
            if (mk) return 64 * r + (__ffsll((long long)mk) - 1);
        }
        return -1;
    }
};

// merge over the first RR registers of a wider list (every entry at 64 RR and beyond is invalid before and after)
template <int RR, int R>
__device__ __forceinline__ void merge_prefix(WaveList<R> &wl, u64 key, uint32_t ef, u64 *perm, int lane, u64 new_flag) {
    static_assert(RR <= R, "prefix of the list");
    WaveList<RR> t;
#pragma unroll
    for (int r = 0; r < RR; r++) t.L[r] = wl.L[r];
    t.n_cur = wl.n_cur;
    t.last_key = wl.last_key;
    t.merge(key, ef, perm, lane, new_flag);
#pragma unroll
    for (int r = 0; r < RR; r++) wl.L[r] = t.L[r];
    wl.n_cur = t.n_cur;
    wl.last_key = t.last_key;
}

// LDS visited table (IntSet::insert, results.rs:101-103): open addressing over BUCKETS of four
// 32-bit slots.  One ds_read_b128 fetches the home bucket, the four compares run in registers and
// a single ds_cmpst claims the first empty slot, so an insert is two LDS round trips whatever the
// load; the classic one-slot linear probe needed one round trip per probe and the wave iterated as
// long as its unluckiest lane (4-5 rounds at 30 % load).  Slots fill left to right and never empty,
// ids within one adjacency row are distinct, so "absent from the bucket, first empty slot claimed"
// is an exact insert.  Returns true when id was not present.
// read-only membership test of the same table (speculative evaluation: nothing may be inserted yet)
__device__ __forceinline__ bool visited_contains(const uint32_t *tab, uint32_t hmask, uint32_t slots_log2,
                                                 uint32_t id) {
    const uint32_t bmask = hmask >> 2;
    uint32_t b = (id * 0x9E3779B1u) >> (32 - (slots_log2 - 2));
    while (true) {
        const uint4 bk = *reinterpret_cast<const uint4 *>(tab + 4 * b);
        if (bk.x == id || bk.y == id || bk.z == id || bk.w == id) return true;
        if (bk.x == HX_EMPTY_SLOT || bk.y == HX_EMPTY_SLOT || bk.z == HX_EMPTY_SLOT || bk.w == HX_EMPTY_SLOT)
            return false;
        b = (b + 1) & bmask;
    }
}

__device__ __forceinline__ bool visited_insert(uint32_t *tab, uint32_t hmask, uint32_t slots_log2,
                                               uint32_t id) {
    const uint32_t bmask = hmask >> 2;
    uint32_t b = (id * 0x9E3779B1u) >> (32 - (slots_log2 - 2));
    while (true) {
        const uint4 bk = *reinterpret_cast<const uint4 *>(tab + 4 * b);
        if (bk.x == id || bk.y == id || bk.z == id || bk.w == id) return false;
        int j = -1;
        if (bk.x == HX_EMPTY_SLOT)
            j = 0;
        else if (bk.y == HX_EMPTY_SLOT)
            j = 1;
        else if (bk.z == HX_EMPTY_SLOT)
            j = 2;
        else if (bk.w == HX_EMPTY_SLOT)
            j = 3;
        if (j < 0) {
            b = (b + 1) & bmask;  // bucket full: next bucket
            continue;
        }
        const uint32_t old = atomicCAS(&tab[4 * b + j], HX_EMPTY_SLOT, id);
        if (old == HX_EMPTY_SLOT) return true;
        // another lane of this wave took that slot in the same round: look at the bucket again
    }
}

}  // namespace hx
