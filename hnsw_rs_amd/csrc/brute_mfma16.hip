// brute_mfma16.hip -- exhaustive ground truth over f16-resident rows (option "rows_f16", DESIGN.md sections 36 and 38) on
// the binary16 matrix cores of gfx950: hx_row_norms16_kernel, hx_brute_mfma16_kernel, hx_pair_distance16_kernel, their
// launchers, and nothing else (libhnsw_mi355x_truth16.so).  The phases and the contract are brute_mfma.hip's: norms, a
// SCREEN by the score s(x) = |x|^2 - 2 x.q that keeps a lane's MF_K2 best by (score, id), the host's merge to k + 8, the
// reference's own distances of the survivors (rows16.inc: the stored row widened exactly into FullVec::distance's single
// f32 chain) and the final (dist, id) sort.  The answer is that of the plain f32 index over the widened rows.
//
// What the screen computes.  v_mfma_f32_32x32x16_f16 takes binary16 operands and accumulates in f32; a product of two
// binary16 values is exact in f32.  The stored row IS an operand: a lane's 16-byte piece holds the 8 halves of row
// lane % 32 and k-block lane / 32.  The query is f32 and is NOT rounded: per query it is scaled by the power of two 2^-e
// that brings its largest |component| into [1, 2) (exact), and every scaled component c is split into three binary16
// planes
//     hi = rn16(c),   mid = rn16((c - hi) 2^11),   lo = rn16((c - hi - mid 2^-11) 2^22)
// (each difference is exact in f32: a value minus its rounding to a coarser grid).  A plane value that would be a
// binary16 subnormal is set to zero instead, so no subnormal operand reaches the instruction from the query side; what
// the three planes leave of c is below 2^-35 whether or not a plane was zeroed (|c - hi| <= 2^-11, the next plane
// leaves at most 2^-12 of that, the third 2^-13 of that; a zeroed plane leaves less than 2^-14 of its own scale).  With
// three accumulators per tile
//     x.q = 2^e (acc_hi + (2^-11 acc_mid + 2^-22 acc_lo)),        score = |x|^2 - 2 x.q.
//
// The declared bound is E16 = 4 E, E = 1.01 (d + 2) 2^-24 max_x (|x|^2 + 2 sum|x_i||q_i|) as tests/ground_truth_inputs.py
// derives it for f32 sums in ANY order.  The factor 4 is an allowance, not a measurement: the products are exact, but the
// instruction's rounding of its 16-term sums is not documented (truncation instead of rounding to nearest doubles the
// unit u: one factor 2), and the recombination adds two roundings of terms no larger than the dot product plus the split
// residual, d 2^-35 max|x_i| max|q_i|, beside E's (d + 2) 2^-24 of the same magnitudes (together well inside the second
// factor 2).  A query whose margin (ground_truth_inputs.margin) is above 4 must equal the exact answer, ids and
// distance bits; beyond it the result is k distinct stored ids with exact distances in order.
//
// Range.  Whether the matrix instruction flushes binary16 subnormals is not assumed: the norms kernel flags a row that
// holds one, and the host answers such a call by the exact scan (ground_truth.cpp), as it does a query whose largest
// |component| is outside [2^-48, 2^40].  Inside, 2^-e and 2^(e+1) are normal f32 values.
//
// Shape.  The f32 kernel is bound by its matrix instruction; this one, at sixteen times the rate and half the bytes, has
// by arithmetic the bytes of the rows as its first roof, which every 32-query column tile reads once (measured, DESIGN.md
// section 38, it reaches neither roof: 52 TFLOP/s; the B reads from LDS and one wave per SIMD are what to look at next).
// So a 256-thread workgroup owns NT = 2
// column tiles wherever their planes fit in LDS (3 planes x 64 queries x (2 d + 16) B: d <= 416) and every A piece a lane
// fetches feeds six MFMAs (2 tiles x 3 planes) into six independent accumulators (96 registers) -- half the row traffic
// of a 32-query tile; wider rows (d = 768: 149 KB for one tile) get NT = 1.  Points never touch LDS and are never
// converted: each lane streams pieces 2 t + lane / 32 of its row straight from HBM into the A operand, MF_CH pieces per
// stage, the next stage in flight while the current one feeds the MFMAs.  Rows are zero-padded to 16 B, so every d is
// served; a half-wave without a piece left (odd piece count) feeds zeros against the zero piece behind the query's row.
// The planes' rows are an odd number of 16-byte pieces long, so the 32 rows of a B read start in 32 different bank groups.
//
// Built without packed-f32 instructions (Makefile), like every kernel that widens f16 rows into the reference's chain.

#include <hip/hip_runtime.h>

#include "launch.h"
#include "search_common.h"

namespace hx {

#include "rows16.inc"

typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));

static constexpr int MF_K2 = 20;  // candidates kept per lane and column tile: brute_mfma_k2(), the host's merge reads both alike
static constexpr int MF_CH = 8;   // 16-byte pieces per lane in flight per stage

// pieces of a plane's row in LDS: the row's own, at least one zero piece behind them, an odd count
__host__ __device__ inline uint32_t plane_pieces(uint32_t np) { return (np + 1) | 1u; }

template <int NT>
__host__ __device__ inline size_t mfma16_lds(uint32_t np) {
    return (size_t)3 * NT * 32 * plane_pieces(np) * 16 + NT * 32 * 4 + 4 * 32 * 4;
}

// xn[i] = |x_i|^2, one left-to-right f32 chain over the widened elements (the padding adds +0); xinfo[i] = the largest
// |x_ie| widened, as its f32 bit pattern, with bit 31 set when the row holds a nonzero binary16 subnormal
__global__ void __launch_bounds__(256)
hx_row_norms16_kernel(const uint8_t *X, uint32_t N, uint32_t np, float *xn, uint32_t *xinfo) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const u32x4 *r = reinterpret_cast<const u32x4 *>(X + (size_t)i * np * 16);
    float s = 0.0f;
    uint32_t m = 0, sub = 0;
    for (uint32_t p = 0; p < np; p++) {
        const u32x4 w = r[p];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const uint32_t b = (w[e >> 1] >> (16 * (e & 1))) & 0x7FFFu;
            const float x = (float)__builtin_bit_cast(_Float16, (uint16_t)b);
            s += x * x;
            m = max(m, b);
            sub |= (b & 0x7C00u) == 0 && b != 0;
        }
    }
    xn[i] = s;
    xinfo[i] = __float_as_uint((float)__builtin_bit_cast(_Float16, (uint16_t)m)) | (sub << 31);
}

// rn16(r), or zero where that is a binary16 subnormal
__device__ __forceinline__ _Float16 plane_value(float r) {
    const _Float16 h = (_Float16)r;
    return (__builtin_bit_cast(uint16_t, h) & 0x7C00u) ? h : (_Float16)0.0f;
}

// One wave stages one query: its planes to row `r` of the three plane arrays, 2^(e+1) to qscale[r].  A row beyond nq is zeros.
__device__ __forceinline__ void stage_planes(const float *q, bool valid, uint32_t d, uint32_t ldp, uint32_t plane_stride,
                                             v8h *planes, float *qscale, uint32_t r, uint32_t lane) {
    uint32_t m = 0;
    if (valid)
        for (uint32_t e = lane; e < d; e += 64) m = max(m, __float_as_uint(q[e]) & 0x7FFFFFFFu);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
    // e: the exponent of the largest |component| (the host sends only queries whose e lies in [-48, 40], or zeros)
    const int e = m == 0 ? 0 : min(126, max(-126, (int)(m >> 23) - 127));
    const float down = __uint_as_float((uint32_t)(127 - e) << 23);
    if (lane == 0) qscale[r] = __uint_as_float((uint32_t)(128 + e) << 23);
    for (uint32_t p = lane; p < ldp; p += 64) {
        v8h hi, mid, lo;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t el = 8 * p + i;
            const float c = (valid && el < d) ? q[el] * down : 0.0f;
            hi[i] = plane_value(c);
            const float r1 = c - (float)hi[i];
            mid[i] = plane_value(r1 * 2048.0f);
            const float r2 = r1 - (float)mid[i] * (1.0f / 2048.0f);
            lo[i] = plane_value(r2 * 4194304.0f);
        }
        v8h *at = planes + (size_t)r * ldp + p;
        at[0] = hi;
        at[plane_stride] = mid;
        at[2 * (size_t)plane_stride] = lo;
    }
}

// (score, id) into a lane's list of its MF_K2 best, as brute_mfma.hip keeps it: the current worst goes -- of the slots
// that tie at the threshold the one with the largest id (an empty slot holds the largest of all).  Ids arrive in
// increasing order and an equal score is not taken, so among equal scores the lowest ids stay: the exact order.
__device__ __forceinline__ void keep_best(float (&bs)[MF_K2], uint32_t (&bi)[MF_K2], float &thr, float sc, uint32_t id) {
    uint32_t worst = 0;
#pragma unroll
    for (int t = 0; t < MF_K2; t++)
        if (bs[t] == thr) worst = max(worst, bi[t]);
    bool done = false;
#pragma unroll
    for (int t = 0; t < MF_K2; t++) {
        if (!done && bs[t] == thr && bi[t] == worst) {
            bs[t] = sc;
            bi[t] = id;
            done = true;
        }
    }
    float mx = bs[0];
#pragma unroll
    for (int t = 1; t < MF_K2; t++) mx = fmaxf(mx, bs[t]);
    thr = mx;
}

// grid (nseg, ceil(ntiles / NT)); out_s / out_i: [ntiles][nseg][4][64][MF_K2], a column tile's lists where the f32 kernel
// puts them
template <int NT>
__global__ void __launch_bounds__(256)
hx_brute_mfma16_kernel(const uint8_t *X, const float *xn, uint32_t N, uint32_t d, uint32_t np, const float *Q, uint32_t nq,
                       uint32_t ntiles, uint32_t nseg, float *out_s, uint32_t *out_i) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t ldp = plane_pieces(np), plane_stride = NT * 32 * ldp;
    v8h *planes = reinterpret_cast<v8h *>(smem);                        // [3][NT * 32][ldp]
    float *qscale = reinterpret_cast<float *>(planes + 3 * (size_t)plane_stride);  // [NT * 32]: 2^(e + 1)
    float *xns = qscale + NT * 32;                                      // [4 waves][32] norms of the current tile
    const uint32_t seg = blockIdx.x, tile0 = blockIdx.y * NT;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t j = lane & 31, hi = lane >> 5;
    for (uint32_t r = wave; r < NT * 32; r += 4) {
        const uint32_t qi = tile0 * 32 + r;
        stage_planes(Q + (size_t)(qi < nq ? qi : 0) * d, qi < nq, d, ldp, plane_stride, planes, qscale, r, lane);
    }
    __syncthreads();
    // ---- this wave's points: a quarter of the segment, in tiles of 32 ----
    const uint64_t per_seg = ((uint64_t)N + nseg - 1) / nseg;
    const uint64_t s_lo = per_seg * seg, s_hi = min((uint64_t)N, s_lo + per_seg);
    const uint64_t per_w = (((s_hi > s_lo ? s_hi - s_lo : 0) + 3) / 4 + 31) / 32 * 32;
    const uint64_t w_lo = s_lo + per_w * wave, w_hi = min(s_hi, w_lo + per_w);
    float bs[NT][MF_K2], thr[NT], qs[NT];
    uint32_t bi[NT][MF_K2];
#pragma unroll
    for (int c = 0; c < NT; c++) {
#pragma unroll
        for (int t = 0; t < MF_K2; t++) {
            bs[c][t] = __builtin_inff();
            bi[c][t] = HX_EMPTY_SLOT;
        }
        thr[c] = __builtin_inff();
        qs[c] = qscale[32 * c + j];
    }
    const uint32_t nmine = (np + 1 - hi) >> 1;  // pieces 2 t + hi < np
    const uint32_t nmax = (np + 1) >> 1;
    const v8h *brow = planes + (size_t)j * ldp + hi;
    for (uint64_t p0 = w_lo; p0 < w_hi; p0 += 32) {
        const uint64_t row = p0 + j;
        const bool rv = row < w_hi;
        const u32x4 *xr = reinterpret_cast<const u32x4 *>(X + (size_t)(rv ? row : w_lo) * np * 16) + hi;
        if (lane < 32) xns[wave * 32 + lane] = rv ? xn[row] : __builtin_inff();
        v16f acc[NT][3];
#pragma unroll
        for (int c = 0; c < NT; c++)
#pragma unroll
            for (int pl = 0; pl < 3; pl++)
#pragma unroll
                for (int v = 0; v < 16; v++) acc[c][pl][v] = 0.0f;
        u32x4 a_cur[MF_CH], a_nxt[MF_CH];
        auto fetch = [&](u32x4 (&w)[MF_CH], uint32_t t0) __attribute__((always_inline)) {
#pragma unroll
            for (int c = 0; c < MF_CH; c++) {
                const uint32_t t = t0 + c;
                const u32x4 zero = {0u, 0u, 0u, 0u};
                w[c] = (t < nmine && rv) ? xr[2 * t] : zero;
            }
        };
        fetch(a_cur, 0);
        // both halves of the wave run the same nmax steps (MFMA is a whole-wave instruction)
        for (uint32_t t0 = 0; t0 < nmax; t0 += MF_CH) {
            if (t0 + MF_CH < nmax) fetch(a_nxt, t0 + MF_CH);
#pragma unroll
            for (int c = 0; c < MF_CH; c++) {
                const uint32_t t = t0 + c;
                if (t < nmax) {  // wave-uniform
                    const v8h a = __builtin_bit_cast(v8h, a_cur[c]);
#pragma unroll
                    for (int ct = 0; ct < NT; ct++)
#pragma unroll
                        for (int pl = 0; pl < 3; pl++) {
                            const v8h b = brow[(size_t)pl * plane_stride + (size_t)ct * 32 * ldp + 2 * t];
                            acc[ct][pl] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[ct][pl], 0, 0, 0);
                        }
                }
            }
#pragma unroll
            for (int c = 0; c < MF_CH; c++) a_cur[c] = a_nxt[c];
        }
        wave_fence();  // the tile's norms are in LDS (own wave)
        // acc[..][v] belongs to point m = (v % 4) + 8 (v / 4) + 4 hi of the tile and query j of column tile ct
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const v4f n4 = *reinterpret_cast<const v4f *>(xns + wave * 32 + 8 * g + 4 * hi);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t id = (uint32_t)(p0 + 8 * g + 4 * hi + u);
#pragma unroll
                for (int ct = 0; ct < NT; ct++) {
                    const int v = 4 * g + u;
                    const float dot = acc[ct][0][v] + (acc[ct][1][v] * (1.0f / 2048.0f) + acc[ct][2][v] * (1.0f / 4194304.0f));
                    const float sc = n4[u] - qs[ct] * dot;
                    if (sc < thr[ct]) keep_best(bs[ct], bi[ct], thr[ct], sc, id);
                }
            }
        }
    }
#pragma unroll
    for (int ct = 0; ct < NT; ct++) {
        if (tile0 + ct >= ntiles) continue;
        const size_t o = ((((size_t)(tile0 + ct) * nseg + seg) * 4 + wave) * 64 + lane) * MF_K2;
#pragma unroll
        for (int t = 0; t < MF_K2; t++) {
            out_s[o + t] = bs[ct][t];
            out_i[o + t] = bi[ct][t];
        }
    }
}

// exact FullVec::distance (full.rs:23-29) of (query, point) pairs over f16 rows: one lane per pair, the stored row
// widened exactly into the single left-to-right chain (rows16.inc)
__global__ void __launch_bounds__(256)
hx_pair_distance16_kernel(const uint8_t *X, uint32_t d, uint32_t np, const float *Q, const uint32_t *qidx,
                          const uint32_t *pidx, uint64_t n, float *out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = pidx[i];
    if (p == HX_EMPTY_SLOT) {
        out[i] = __builtin_inff();
        return;
    }
    out[i] = __builtin_sqrtf(f16_row_lane(X + (size_t)p * np * 16, d, np, Q + (size_t)qidx[i] * d));
}

namespace {

bool f16_view(const DevView &v) {
    if (v.kind == HNSW_VEC_F32 && v.rows16 && v.row_stride == f16_row_stride(v.dim)) return true;
    set_error("the f16 MFMA scan: the snapshot does not hold f16 rows");
    return false;
}

template <int NT>
int launch_mfma16(const DevView &v, const float *d_xn, const float *d_Q, uint32_t nq, uint32_t nseg, float *out_s,
                  uint32_t *out_i, hipStream_t stream) {
    const uint32_t np = v.row_stride >> 4, ntiles = (nq + 31) / 32;
    return launch_checked({"f16 MFMA scan launch", "the f16 MFMA scan stages 32 queries in three planes in LDS: dimension %zu is too large", v.dim},
                          hx_brute_mfma16_kernel<NT>, dim3(nseg, (ntiles + NT - 1) / NT), dim3(256), mfma16_lds<NT>(np), stream,
                          v.rows, d_xn, v.n_points, v.dim, np, d_Q, nq, ntiles, nseg, out_s, out_i);
}

}  // namespace

int launch_row_norms16(const DevView &v, float *d_xn, uint32_t *d_xinfo, hipStream_t stream) {
    if (!f16_view(v)) return HNSW_ERR_ARG;
    return launch_checked({"f16 row norms launch"}, hx_row_norms16_kernel, dim3((v.n_points + 255) / 256), dim3(256), 0, stream,
                          v.rows, v.n_points, v.row_stride >> 4, d_xn, d_xinfo);
}

// out_s / out_i: [ntiles][nseg][4][64][brute_mfma_k2()], as launch_brute_mfma's
int launch_brute_mfma16(const DevView &v, const float *d_xn, const float *d_Q, uint32_t nq, uint32_t nseg, float *out_s,
                        uint32_t *out_i, hipStream_t stream) {
    static_assert(MF_K2 == 20, "the host merges these lists as it merges the f32 kernel's (brute_mfma_k2)");
    if (!f16_view(v)) return HNSW_ERR_ARG;
    if (mfma16_lds<2>(v.row_stride >> 4) <= 160 * 1024) return launch_mfma16<2>(v, d_xn, d_Q, nq, nseg, out_s, out_i, stream);
    return launch_mfma16<1>(v, d_xn, d_Q, nq, nseg, out_s, out_i, stream);
}

int launch_pair_distance16(const DevView &v, const float *d_Q, const uint32_t *d_qidx, const uint32_t *d_pidx, uint64_t n,
                           float *d_out, hipStream_t stream) {
    if (!f16_view(v)) return HNSW_ERR_ARG;
    if (n == 0) return HNSW_OK;
    return launch_checked({"f16 pair distance launch"}, hx_pair_distance16_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0,
                          stream, v.rows, v.dim, v.row_stride >> 4, d_Q, d_qidx, d_pidx, n, d_out);
}

}  // namespace hx
