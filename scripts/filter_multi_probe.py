"""Per-query masks on the bench's index (1M x 100d, m 16, ef_cons 32, on-device build, as bench.py builds it): one
hnsw_search_batch_filtered_multi call of 1024 queries under G masks against the loop it replaces, G
hnsw_search_batch_filtered calls over the same query groups.  Both kinds, n 10, ef 64, G in {1, 4, 16, 64, 256}, the
queries dealt round-robin to the masks, two mask families:
  random     G independent masks of selectivity 0.2: every mask on the graph path;
  partition  the ids dealt to G tenants (selectivity 1 / G): the graph path up to G = 4, the exact path from
             G = 16 on (62500 ids <= the default "filter_exact_max" of 65536).
The masks are packed once, outside the clock, and both forms go through the C entry points directly (the Python
mirror packs its masks in every call): the time is the host clock around the call(s), each of which ends in a device
synchronise -- uploads, kernels, result copy.  Per point: the median and the spread of REPS repeats of each form, taken
alternately in one process after a warm-up of both; the queries per path; and whether both forms gave identical ids,
distances, counts, counters and paths.

usage: python scripts/filter_multi_probe.py OUT.json [--quick]   (GPU; --quick: G in {1, 16} only)"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402
from hnsw_rs_amd import _lib  # noqa: E402

N, D, M, EFC, B, TOPN, EF = 1_000_000, 100, 16, 32, 1024, 10, 64
GS = [1, 4, 16, 64, 256]
REPS = 3
W = (N + 63) // 64


def build(kind):
    vs = H.synth_rows(0, 0x5EED0001, 0, N, D, 16)
    idx = H.HNSW.new(M, EFC, D, kind)
    idx.insert_bulk_device(vs, 16, False)
    idx.upload()
    return idx


def packed(family, G, rng):
    """-> words [G, W] uint64"""
    out = np.zeros((G, W), dtype=np.uint64)
    tenant = rng.integers(0, G, N) if family == "partition" else None
    for g in range(G):
        out[g] = H.pack_allow(tenant == g if family == "partition" else rng.random(N) < 0.2)[0]
    return out


class Outputs:
    def __init__(self, nq):
        self.ids = np.zeros((nq, TOPN), dtype=np.uint32)
        self.dists = np.zeros((nq, TOPN), dtype=np.float32)
        self.counts = np.zeros(nq, dtype=np.uint32)
        self.stats = np.zeros((nq, 4), dtype=np.int32)
        self.paths = np.zeros(nq, dtype=np.uint8)

    def args(self):
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
        return (p(self.ids, C.c_uint32), p(self.dists, C.c_float), p(self.counts, C.c_uint32),
                C.cast(self.stats.ctypes.data, C.POINTER(_lib.QueryStats)), p(self.paths, C.c_uint8))

    def same(self, o):
        return all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                  b.view(np.uint32) if b.dtype == np.float32 else b)
                   for a, b in ((self.ids, o.ids), (self.dists, o.dists), (self.counts, o.counts),
                                (self.stats, o.stats), (self.paths, o.paths)))


def point(idx, qs, words, G):
    L = _lib.lib()
    f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    mask_of = (np.arange(B) % G).astype(np.uint32)
    multi_out = Outputs(B)
    m_args = multi_out.args()

    def multi():
        H.hnsw.check(L.hnsw_search_batch_filtered_multi(idx._h, qs.ctypes.data_as(f32p), B, TOPN, EF,
                                                        words.ctypes.data_as(u64p), G, N, mask_of.ctypes.data_as(u32p),
                                                        *m_args))

    # the loop: group g's queries gathered once, outside the clock, as a caller that splits its batch holds them
    groups = [np.flatnonzero(mask_of == g) for g in range(G)]
    g_qs = [np.ascontiguousarray(qs[r]) for r in groups]
    g_out = [Outputs(len(r)) for r in groups]
    g_args = [o.args() for o in g_out]

    def loop():
        for g in range(G):
            H.hnsw.check(L.hnsw_search_batch_filtered(idx._h, g_qs[g].ctypes.data_as(f32p), len(groups[g]), TOPN, EF,
                                                      words[g].ctypes.data_as(u64p), N, *g_args[g]))

    multi()
    loop()
    t_m, t_l = [], []
    for _ in range(REPS):
        for fn, t in ((multi, t_m), (loop, t_l)):
            t0 = time.perf_counter()
            fn()
            t.append(1e3 * (time.perf_counter() - t0))
    gathered = Outputs(B)
    for r, o in zip(groups, g_out):
        for name in ("ids", "dists", "counts", "stats", "paths"):
            getattr(gathered, name)[r] = getattr(o, name)
    return dict(multi_ms=float(np.median(t_m)), multi_ms_all=t_m, loop_ms=float(np.median(t_l)), loop_ms_all=t_l,
                paths={str(k): int((multi_out.paths == k).sum()) for k in (0, 1, 2)},
                identical=bool(multi_out.same(gathered)))


def main():
    out_path = sys.argv[1]
    gs = [1, 16] if "--quick" in sys.argv else GS
    res = {"shape": dict(n=N, d=D, m=M, ef_cons=EFC, batch=B, topn=TOPN, ef=EF, reps=REPS,
                         timing="host ms for 1024 queries: one multi call / the loop of G single-mask calls; median of "
                                "reps, alternating, every call ends in a device synchronise; masks packed outside"),
           "points": []}
    for kind_name in ("f32", "quant8"):
        t0 = time.time()
        idx = build(H.VEC_F32 if kind_name == "f32" else H.VEC_QUANT8)
        print("%s index built in %.1f s" % (kind_name, time.time() - t0), flush=True)
        qs = np.ascontiguousarray(H.synth_rows(0, 0x5EED0002, 0, B, D, 16))
        for family in ("random", "partition"):
            rng = np.random.default_rng(2025)
            for G in gs:
                words = packed(family, G, rng)
                p = dict(kind=kind_name, family=family, G=G, **point(idx, qs, words, G))
                res["points"].append(p)
                print(json.dumps(p), flush=True)
        del idx
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
