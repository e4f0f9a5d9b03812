"""A label range AND a row of a resident mask set in one call, on the bench's index (1M x 100d, m 16, ef_cons 32,
on-device build, as bench.py builds it; the setup of scripts/label_probe.py): 1024 queries, both kinds, n 10, ef 64.
  (a)  tenants x ACL: labels = id % G, 16 random rows of selectivity 0.5 in a resident set, query i under
       (row i % 16, [i % G, i % G]), for G in {4, 64, 1024} -- hnsw_search_batch_filtered_set_range against
       hnsw_search_batch_filtered_multi with the 1024 conjunction masks packed afresh inside the clock, the only way to
       say it without this call.  The paths taken are recorded per point.
  (b)  the same rows with a per-query sliding window of selectivity 0.2 over timestamps drawn from [0, 1M).
  (c)  the planner's host time alone, first call after set_labels and warm: the same call with ef = 257, which the
       planner refuses (HNSW_ERR_ARG: a triple on the graph path) after it has counted every triple and before the
       device is touched.  Recorded for (a) and (b), at the default "filter_exact_max".
The forms alternate in one process after a warm-up of each; per point the median and all REPS repeats, host clock around
the call, each of which ends in a device synchronise; whether both forms gave identical ids, distances, counts, counters
and paths.

usage: python scripts/filter_set_range_probe.py OUT.json [--quick]   (GPU; --quick: G in {4, 64}, and (b))"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402
from hnsw_rs_amd import _lib  # noqa: E402
from scripts.filter_multi_probe import B, D, EF, N, TOPN, W, Outputs, build  # noqa: E402
from scripts.label_probe import REPS, alternate, ms, timed  # noqa: E402

GS = [4, 64, 1024]
ROWS = 16
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def point(idx, qs, s, rows_b, labels, lo, hi, case):
    """one comparison on labels already set: -> timings, paths, identity, the planner's host time first and warm"""
    L, check = _lib.lib(), H.hnsw.check
    mask_of = (np.arange(B) % ROWS).astype(np.uint32)
    each = np.arange(B, dtype=np.uint32)
    c_out, m_out = Outputs(B), Outputs(B)
    c_args, m_args = c_out.args(), m_out.args()
    q, mo, plo, phi = (qs.ctypes.data_as(f32p), mask_of.ctypes.data_as(u32p), lo.ctypes.data_as(u32p),
                       hi.ctypes.data_as(u32p))

    def planner():  # refused after the planner ran, before the device is touched
        rc = L.hnsw_search_batch_filtered_set_range(idx._h, q, B, TOPN, 257, s, mo, plo, phi, *c_args)
        if rc != _lib.ERR_ARG:
            raise RuntimeError("the planner probe expects HNSW_ERR_ARG, got %d" % rc)

    def combined():
        check(L.hnsw_search_batch_filtered_set_range(idx._h, q, B, TOPN, EF, s, mo, plo, phi, *c_args))

    def multi_fresh():  # the conjunction of every query as a mask of its own, made for this call
        words = np.stack([H.pack_allow(rows_b[i % ROWS] & (labels >= lo[i]) & (labels <= hi[i]))[0] for i in range(B)])
        check(L.hnsw_search_batch_filtered_multi(idx._h, q, B, TOPN, EF, words.ctypes.data_as(u64p), B, N,
                                                 each.ctypes.data_as(u32p), *m_args))

    on_graph = True
    try:
        t_plan_first = ms(planner)  # with the sort of the column's keys
        t_plan = [ms(planner) for _ in range(REPS)]
    except RuntimeError:  # every triple is on the exact path: ef' = 257 is allowed, there is no call that stops early
        on_graph, t_plan_first, t_plan = False, None, []
    t_first = ms(combined)  # the column's whole copy (and the sort, when the planner probe did not run)
    t = alternate((("set_range", combined), ("multi_fresh_masks", multi_fresh)))
    out = dict(case=case, paths={str(k): int((c_out.paths == k).sum()) for k in (0, 1, 2)},
               identical=bool(c_out.same(m_out)), first_call_ms=t_first, planner_first_ms=t_plan_first,
               planner_warm_ms=float(np.median(t_plan)) if on_graph else None, planner_warm_ms_all=t_plan,
               triples=int(len(set(zip(mask_of.tolist(), lo.tolist(), hi.tolist())))),
               column_hbm_bytes=4 * N, set_hbm_bytes=8 * W * ROWS, masks_hbm_bytes=8 * W * B)
    return timed(out, t)


def main():
    out_path = sys.argv[1]
    gs = [4, 64] if "--quick" in sys.argv else GS
    res = {"shape": dict(n=N, d=D, batch=B, topn=TOPN, ef=EF, reps=REPS, rows=ROWS,
                         timing="host ms for 1024 queries, one call of each form; median of reps after a warm-up of "
                                "each, the forms alternating, every call ends in a device synchronise; the set warm; "
                                "the multi form packs its 1024 conjunction masks inside the clock; planner_*: the call "
                                "with ef = 257, refused after the planner and before the device"),
           "points": []}
    L, check = _lib.lib(), H.hnsw.check
    for kind_name in ("f32", "quant8"):
        t0 = time.time()
        idx = build(H.VEC_F32 if kind_name == "f32" else H.VEC_QUANT8)
        print("%s index built in %.1f s" % (kind_name, time.time() - t0), flush=True)
        qs = np.ascontiguousarray(H.synth_rows(0, 0x5EED0002, 0, B, D, 16))
        rng = np.random.default_rng(2027)
        rows_b = rng.random((ROWS, N)) < 0.5
        words = np.stack([H.pack_allow(r)[0] for r in rows_b])
        s = C.c_void_p()
        check(L.hnsw_mask_set_create(idx._h, ROWS, N, words.ctypes.data_as(u64p), C.byref(s)))
        ids = np.arange(N)
        points = []
        for G in gs:
            labels = (ids % G).astype(np.uint32)
            idx.set_labels(labels)
            lo = (np.arange(B) % G).astype(np.uint32)
            points.append(dict(G=G, **point(idx, qs, s, rows_b, labels, lo, lo, "tenants x ACL")))
        stamp = rng.integers(0, N, N).astype(np.uint32)
        idx.set_labels(stamp)
        lo = rng.integers(0, N - N // 5, B).astype(np.uint32)
        hi = (lo + N // 5 - 1).astype(np.uint32)
        points.append(dict(selectivity=0.2, **point(idx, qs, s, rows_b, stamp, lo, hi, "sliding window x ACL")))
        for p in points:
            p = dict(kind=kind_name, **p)
            res["points"].append(p)
            print(json.dumps(p), flush=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
        L.hnsw_mask_set_free(s)
        del idx
    print("wrote", out_path)


if __name__ == "__main__":
    main()
