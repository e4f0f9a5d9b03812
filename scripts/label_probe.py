"""Label-range filtered search on the bench's index (1M x 100d, m 16, ef_cons 32, on-device build, as bench.py builds
it; the setup of scripts/filter_set_probe.py): 1024 queries, both kinds, n 10, ef 64.
  (a), (b)  tenants: labels = id % G, query i under [i % G, i % G], for G in {1, 4, 64, 256, 1024} --
            hnsw_search_batch_filtered_range against hnsw_search_batch_filtered_set on a warm set whose row g is the mask
            {id : id % G == g}.  The planner puts both on the graph path while 1M / G > "filter_exact_max" (65536) and on
            the exact path from there on; the paths taken are recorded per point.
  (c)       a sliding window: labels are timestamps drawn from [0, 1M), query i under a window of its own of
            selectivity 0.2 -- against hnsw_search_batch_filtered_multi with the 1024 masks packed afresh inside the clock,
            the only way to express it without labels.
The forms alternate in one process after a warm-up of each; per point the median and all REPS repeats, host clock around
the call, each of which ends in a device synchronise; whether both forms gave identical ids, distances, counts, counters
and paths; the HBM bytes of the column and of the masks; and the first range call after set_labels (the whole copy of
the column and the planner's sort).

usage: python scripts/label_probe.py OUT.json [--quick]   (GPU; --quick: G in {1, 64}, and (c))"""
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

GS = [1, 4, 64, 256, 1024]
REPS = 3
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def alternate(forms):
    """a warm-up of each form, then REPS repeats, the forms alternating -> {name: [ms]}"""
    for _, fn in forms:
        fn()
    t = {name: [] for name, _ in forms}
    for _ in range(REPS):
        for name, fn in forms:
            t[name].append(ms(fn))
    return t


def timed(out, t):
    for name, v in t.items():
        out[name + "_ms"] = float(np.median(v))
        out[name + "_ms_all"] = v
    return out


def tenants(idx, qs, G):
    L, check = _lib.lib(), H.hnsw.check
    ids = np.arange(N)
    idx.set_labels((ids % G).astype(np.uint32))
    lo = (np.arange(B) % G).astype(np.uint32)
    words = np.stack([H.pack_allow(ids % G == g)[0] for g in range(G)])
    s = C.c_void_p()
    check(L.hnsw_mask_set_create(idx._h, G, N, words.ctypes.data_as(u64p), C.byref(s)))
    r_out, s_out = Outputs(B), Outputs(B)
    r_args, s_args = r_out.args(), s_out.args()

    def ranged():
        check(L.hnsw_search_batch_filtered_range(idx._h, qs.ctypes.data_as(f32p), B, TOPN, EF, lo.ctypes.data_as(u32p),
                                                 lo.ctypes.data_as(u32p), *r_args))

    def under_set():
        check(L.hnsw_search_batch_filtered_set(idx._h, qs.ctypes.data_as(f32p), B, TOPN, EF, s, lo.ctypes.data_as(u32p),
                                               *s_args))

    t_first = ms(ranged)  # the column's whole copy and the planner's sort
    t = alternate((("range", ranged), ("set", under_set)))
    L.hnsw_mask_set_free(s)
    out = dict(case="tenants", G=G, paths={str(k): int((r_out.paths == k).sum()) for k in (0, 1, 2)},
               identical=bool(r_out.same(s_out)), first_range_call_ms=t_first, column_hbm_bytes=4 * N,
               masks_hbm_bytes=8 * W * G)
    return timed(out, t)


def sliding(idx, qs):
    L, check = _lib.lib(), H.hnsw.check
    rng = np.random.default_rng(2026)
    stamp = rng.integers(0, N, N).astype(np.uint32)
    idx.set_labels(stamp)
    lo = rng.integers(0, N - N // 5, B).astype(np.uint32)
    hi = (lo + N // 5 - 1).astype(np.uint32)
    mask_of = np.arange(B, dtype=np.uint32)
    r_out, m_out = Outputs(B), Outputs(B)
    r_args, m_args = r_out.args(), m_out.args()

    def ranged():
        check(L.hnsw_search_batch_filtered_range(idx._h, qs.ctypes.data_as(f32p), B, TOPN, EF, lo.ctypes.data_as(u32p),
                                                 hi.ctypes.data_as(u32p), *r_args))

    def multi_fresh():  # the windows slide: the masks of a call cannot be kept from the one before
        words = np.stack([H.pack_allow((stamp >= lo[i]) & (stamp <= hi[i]))[0] for i in range(B)])
        check(L.hnsw_search_batch_filtered_multi(idx._h, qs.ctypes.data_as(f32p), B, TOPN, EF, words.ctypes.data_as(u64p),
                                                 B, N, mask_of.ctypes.data_as(u32p), *m_args))

    t_first = ms(ranged)
    t = alternate((("range", ranged), ("multi_fresh_masks", multi_fresh)))
    out = dict(case="sliding", selectivity=0.2, paths={str(k): int((r_out.paths == k).sum()) for k in (0, 1, 2)},
               identical=bool(r_out.same(m_out)), first_range_call_ms=t_first, column_hbm_bytes=4 * N,
               masks_hbm_bytes=8 * W * B)
    return timed(out, t)


def main():
    out_path = sys.argv[1]
    gs = [1, 64] if "--quick" in sys.argv else GS
    res = {"shape": dict(n=N, d=D, batch=B, topn=TOPN, ef=EF, reps=REPS,
                         timing="host ms for 1024 queries, one call of each form; median of reps after a warm-up of "
                                "each, the forms alternating, every call ends in a device synchronise; the set warm; "
                                "the sliding case packs its 1024 masks inside the clock"),
           "points": []}
    for kind_name in ("f32", "quant8"):
        t0 = time.time()
        idx = build(H.VEC_F32 if kind_name == "f32" else H.VEC_QUANT8)
        print("%s index built in %.1f s" % (kind_name, time.time() - t0), flush=True)
        qs = np.ascontiguousarray(H.synth_rows(0, 0x5EED0002, 0, B, D, 16))
        for p in [tenants(idx, qs, G) for G in gs] + [sliding(idx, qs)]:
            p = dict(kind=kind_name, **p)
            res["points"].append(p)
            print(json.dumps(p), flush=True)
            with open(out_path, "w") as f:
                json.dump(res, f, indent=1)
        del idx
    print("wrote", out_path)


if __name__ == "__main__":
    main()
