// ground_truth.cpp -- the two ground-truth scans (search_host.h): HBM buffers, one launch per 2048 queries, the
// partial lists copied back and merged on the host.  Every recall figure of the project rests on these two.

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "search_host.h"

namespace hx {

namespace {

constexpr uint64_t BATCH = 2048;  // queries per launch (the MFMA scan: 64 tiles of 32)
using Cands = std::vector<std::pair<float, uint32_t>>;

// The k best of one query's candidates by (dist, id) -- Dist::cmp for non-NaN distances; ids are distinct, so the
// order is total -- written to ids (and dists, if given); what is missing is padded with UINT32_MAX / INFINITY.
void write_best(Cands &cand, uint32_t k, uint32_t *ids, float *dists) {
    const size_t keep = std::min<size_t>(k, cand.size());
    std::partial_sort(cand.begin(), cand.begin() + keep, cand.end());
    for (uint32_t j = 0; j < k; j++) {
        ids[j] = j < keep ? cand[j].second : UINT32_MAX;
        if (dists) dists[j] = j < keep ? cand[j].first : INFINITY;
    }
}

int nan_error(int status) {
    set_error("NaN in a query or a distance");
    return status;
}

}  // namespace

int exact_scan(hnsw_index *h, const float *Q, uint64_t nq, uint32_t k, uint32_t *ids, float *dists) {
    int rc;
    if (h->del.count) {
        // the top k of the undeleted ids: the filtered search's exact path, in the same arithmetic and (dist, id) order
        std::vector<hnsw_query_stats> st(nq);
        Filter scan;
        scan.family = Filter::SCAN;
        if ((rc = search_filtered(h, Q, nq, k, k, scan, true, ids, dists, nullptr, st.data(), nullptr))) return rc;
        for (uint64_t i = 0; i < nq; i++)
            if (st[i].status != HNSW_OK) return nan_error(st[i].status);
        return HNSW_OK;
    }
    if ((rc = ensure_uploaded(h))) return rc;
    const DevView &v = h->dev.view;
    const uint32_t nseg = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(512, (v.n_points + 2047) / 2048));
    const size_t per_query = (size_t)nseg * k;  // a partial list of k per segment
    DevBuf dQ, dIds, dDists, dSt;
    if ((rc = dQ.alloc(BATCH * v.dim * 4)) || (rc = dIds.alloc(BATCH * per_query * 4)) ||
        (rc = dDists.alloc(BATCH * per_query * 4)) || (rc = dSt.alloc(4)))
        return rc;
    std::vector<uint32_t> pid(BATCH * per_query);
    std::vector<float> pd(BATCH * per_query);
    Cands cand;
    for (uint64_t q0 = 0; q0 < nq; q0 += BATCH) {
        const uint64_t nb = std::min(BATCH, nq - q0);
        HIP_TRY(hipMemcpy(dQ.p, Q + q0 * v.dim, nb * v.dim * 4, hipMemcpyHostToDevice));
        if ((rc = cosine_queries(h, dQ.p, nb, nullptr))) return rc;
        HIP_TRY(hipMemset(dSt.p, 0, 4));
        if ((rc = launch_brute_force(v, dQ.as<float>(), nb, k, nseg, dIds.as<uint32_t>(), dDists.as<float>(), dSt.as<int32_t>(),
                                     nullptr)))
            return rc;
        HIP_TRY(hipDeviceSynchronize());
        int32_t st = 0;
        HIP_TRY(hipMemcpy(&st, dSt.p, 4, hipMemcpyDeviceToHost));
        if (st != HNSW_OK) return nan_error(st);
        HIP_TRY(hipMemcpy(pid.data(), dIds.p, nb * per_query * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(pd.data(), dDists.p, nb * per_query * 4, hipMemcpyDeviceToHost));
        for (uint64_t qi = 0; qi < nb; qi++) {
            cand.clear();
            for (size_t j = qi * per_query; j < (qi + 1) * per_query; j++)
                if (pid[j] != UINT32_MAX) cand.emplace_back(pd[j], pid[j]);
            write_best(cand, k, ids + (q0 + qi) * k, dists ? dists + (q0 + qi) * k : nullptr);
        }
    }
    return HNSW_OK;
}

// Ground truth on the matrix cores (brute_mfma.hip): MFMA scores screen every point, the k + 8 best per
// query are re-evaluated in the reference's exact arithmetic and sorted by (dist, id).  Not bit-exact by
// construction (the screen could in principle lose a true neighbour to rounding): exact_scan is the
// exact scan; this one is for ground truth at sizes where the exact scan takes minutes.
int mfma_scan(hnsw_index *h, const float *Q, uint64_t nq, uint32_t k, uint32_t *ids, float *dists) {
    if (h->del.count) {  // the k + 8 re-rank cannot promise k undeleted ids: no ground truth rather than a wrong one
        set_error("hnsw_brute_force_fast refuses while ids are deleted (%llu); hnsw_brute_force excludes them",
                  (unsigned long long)h->del.count);
        return HNSW_ERR_ARG;
    }
    int rc = ensure_uploaded(h);
    if (rc != HNSW_OK) return rc;
    const DevView &v = h->dev.view;
    if (v.kind != HNSW_VEC_F32 || (v.dim & 3u)) {
        set_error("the MFMA scan serves f32 rows whose dimension is a multiple of 4");
        return HNSW_ERR_ARG;
    }
    // A NaN in a query makes every screen score NaN, and `score < threshold` is false for NaN: the screen would
    // keep nothing and the call would return padding ids with status OK where the exact scan reports
    // HNSW_ERR_NAN_INPUT (stored rows cannot hold one: insert rejects them)
    for (uint64_t i = 0; i < nq * (uint64_t)v.dim; i++)
        if (Q[i] != Q[i]) {
            set_error("query %llu: NaN in the query", (unsigned long long)(i / v.dim));
            return HNSW_ERR_NAN_INPUT;
        }
    // (buffers sized for the tiles a launch really has: a 32-query call on a multi-million-point index has one
    // tile and up to 768 segments, not 64 tiles of them)
    const uint32_t ntile_max = (uint32_t)((std::min(BATCH, nq) + 31) / 32);
    // about 768 workgroups per launch (256 CUs, up to three 32-query tiles of a small dimension each), but
    // no segment shorter than a few point tiles per wave; fewer segments = fewer partial lists to merge
    const uint32_t nseg = (uint32_t)std::max<uint64_t>(
        1, std::min<uint64_t>(std::max<uint32_t>(1, 768 / ntile_max), (uint64_t)v.n_points / 4096));
    const uint32_t K2 = brute_mfma_k2(), M = k + 8;
    const size_t per_tile = (size_t)nseg * 4 * 64 * K2;
    DevBuf dQ, dXn, dS, dI, dQi, dPi, dOut, dXa;
    if ((rc = dQ.alloc(BATCH * v.dim * 4)) || (rc = dXn.alloc((size_t)v.n_points * 4)) ||
        (rc = dS.alloc(ntile_max * per_tile * 4)) || (rc = dI.alloc(ntile_max * per_tile * 4)) ||
        (rc = dQi.alloc(BATCH * M * 4)) || (rc = dPi.alloc(BATCH * M * 4)) || (rc = dOut.alloc(BATCH * M * 4)) ||
        (rc = dXa.alloc((size_t)v.n_points * 4)) || (rc = launch_row_norms(v, dXn.as<float>(), dXa.as<uint32_t>(), nullptr)))
        return rc;
    // The screen's guarantee models relative rounding and holds only inside f32's normal range (brute_mfma.hip): a
    // call with a stored row or a query whose largest |component| is not zero and outside [2^-48, 2^40] is the exact
    // scan's.  (Under the cosine option a query is a unit vector by the time the screen reads it.)
    {
        const uint32_t lo = 0x27800000u, hi = 0x53800000u;  // the bit patterns of 2^-48 and 2^40
        auto outside = [&](uint32_t bits) { return bits != 0 && (bits < lo || bits > hi); };
        std::vector<uint32_t> xa((size_t)v.n_points);
        HIP_TRY(hipMemcpy(xa.data(), dXa.p, xa.size() * 4, hipMemcpyDeviceToHost));
        bool exact = false;
        for (size_t i = 0; i < xa.size() && !exact; i++) exact = outside(xa[i]);
        for (uint64_t i = 0; i < nq && !exact && !h->cosine; i++) {
            uint32_t m = 0, w;
            for (uint32_t e = 0; e < v.dim; e++) {
                memcpy(&w, &Q[i * v.dim + e], 4);
                m = std::max(m, w & 0x7FFFFFFFu);
            }
            exact = outside(m);
        }
        if (exact) return exact_scan(h, Q, nq, k, ids, dists);
    }
    std::vector<float> hs(ntile_max * per_tile), hd(BATCH * M);
    std::vector<uint32_t> hi(ntile_max * per_tile), qidx(BATCH * M), pidx(BATCH * M);
    Cands cand;
    for (uint64_t q0 = 0; q0 < nq; q0 += BATCH) {
        const uint64_t nb = std::min(BATCH, nq - q0);
        const uint32_t ntile = (uint32_t)((nb + 31) / 32);
        HIP_TRY(hipMemcpy(dQ.p, Q + q0 * v.dim, nb * v.dim * 4, hipMemcpyHostToDevice));
        if ((rc = cosine_queries(h, dQ.p, nb, nullptr))) return rc;
        if ((rc = launch_brute_mfma(v, dXn.as<float>(), dQ.as<float>(), (uint32_t)nb, nseg, dS.as<float>(), dI.as<uint32_t>(),
                                    nullptr)))
            return rc;
        HIP_TRY(hipMemcpy(hs.data(), dS.p, ntile * per_tile * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(hi.data(), dI.p, ntile * per_tile * 4, hipMemcpyDeviceToHost));
        // per query: the lists of lanes j and j + 32 of every (segment, wave); keep the M best scores
        for (uint64_t qi = 0; qi < nb; qi++) {
            const uint32_t tile = (uint32_t)(qi / 32), j = (uint32_t)(qi % 32);
            cand.clear();
            for (uint32_t sw = 0; sw < nseg * 4; sw++)
                for (uint32_t half = 0; half < 2; half++) {
                    const size_t o = (((size_t)tile * nseg * 4 + sw) * 64 + j + 32 * half) * K2;
                    for (uint32_t t = 0; t < K2; t++)
                        if (hi[o + t] != UINT32_MAX) cand.emplace_back(hs[o + t], hi[o + t]);
                }
            std::fill_n(&qidx[qi * M], M, (uint32_t)qi);
            write_best(cand, M, &pidx[qi * M], nullptr);
        }
        // exact distances of the survivors, in the reference's arithmetic
        HIP_TRY(hipMemcpy(dQi.p, qidx.data(), nb * M * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dPi.p, pidx.data(), nb * M * 4, hipMemcpyHostToDevice));
        if ((rc = launch_pair_distance(v, dQ.as<float>(), dQi.as<uint32_t>(), dPi.as<uint32_t>(), nb * M, dOut.as<float>(), nullptr)))
            return rc;
        HIP_TRY(hipMemcpy(hd.data(), dOut.p, nb * M * 4, hipMemcpyDeviceToHost));
        for (uint64_t qi = 0; qi < nb; qi++) {
            cand.clear();
            for (size_t t = qi * M; t < (qi + 1) * M; t++) {
                if (pidx[t] == UINT32_MAX) continue;
                if (hd[t] != hd[t]) return nan_error(HNSW_ERR_NAN_INPUT);
                cand.emplace_back(hd[t], pidx[t]);
            }
            write_best(cand, k, ids + (q0 + qi) * k, dists ? dists + (q0 + qi) * k : nullptr);
        }
    }
    return HNSW_OK;
}

}  // namespace hx
