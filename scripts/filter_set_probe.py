"""Resident mask sets on the bench's index (1M x 100d, m 16, ef_cons 32, on-device build, as bench.py builds it; the
setup of scripts/filter_multi_probe.py): 1024 queries under G masks, both kinds, n 10, ef 64, G in {1, 4, 16, 64, 256},
the queries dealt round-robin to the masks, the mask families *random* (selectivity 0.2: the graph path) and *partition*
(selectivity 1 / G: the exact path from G = 16 on).  Three forms of the same search:
  (a) multi   hnsw_search_batch_filtered_multi: the masks travel with every call (packed once, outside the clock);
  (b) set     hnsw_search_batch_filtered_set on a warm set: in HBM, counted, compacted;
  (c) device  hnsw_search_batch_filtered_device + _finish, queries, mask_of and outputs in HBM (torch tensors); every
              query by the graph path, as that form's contract says, so on the partition family from G = 16 on it does
              other work than (a) and (b) and is checked against the set with "filter_exact_max" = -1 instead.
The forms alternate in one process after a warm-up of each; per point the median and the range of REPS repeats, host
clock around the call(s), each of which ends in a device synchronise; whether (a) and (b) gave identical ids,
distances, counts, counters and paths; the cost of creating the set (host only) and of its first call; and the cost of
a 1000-id update of one row followed by one call.

usage: python scripts/filter_set_probe.py OUT.json [--quick]   (GPU; --quick: G in {1, 16} only)"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402
from hnsw_rs_amd import _lib  # noqa: E402
from scripts.filter_multi_probe import B, D, EF, GS, N, TOPN, Outputs, build, packed  # noqa: E402

REPS = 3
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def point(idx, qs, words, G):
    import torch
    L = _lib.lib()
    check = H.hnsw.check
    mask_of = (np.arange(B) % G).astype(np.uint32)
    a_out, b_out = Outputs(B), Outputs(B)
    a_args, b_args = a_out.args(), b_out.args()

    def multi():
        check(L.hnsw_search_batch_filtered_multi(idx._h, qs.ctypes.data_as(f32p), B, TOPN, EF, words.ctypes.data_as(u64p),
                                                 G, N, mask_of.ctypes.data_as(u32p), *a_args))

    s = C.c_void_p()
    t_create = ms(lambda: check(L.hnsw_mask_set_create(idx._h, G, N, words.ctypes.data_as(u64p), C.byref(s))))

    def under_set():
        check(L.hnsw_search_batch_filtered_set(idx._h, qs.ctypes.data_as(f32p), B, TOPN, EF, s, mask_of.ctypes.data_as(u32p),
                                               *b_args))

    dev = torch.device("cuda:0")
    dQ = torch.from_numpy(qs).to(dev)
    d_mo = torch.from_numpy(mask_of.view(np.int32)).to(dev)
    d_ids = torch.zeros((B, TOPN), dtype=torch.int32, device=dev)
    d_d = torch.zeros((B, TOPN), dtype=torch.float32, device=dev)
    d_c = torch.zeros(B, dtype=torch.int32, device=dev)
    d_s = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    d_args = (idx._h, dQ.data_ptr(), B, TOPN, EF, s, d_mo.data_ptr(), d_ids.data_ptr(), d_d.data_ptr(), d_c.data_ptr(),
              d_s.data_ptr(), None)
    torch.cuda.synchronize(dev)

    def device():
        check(L.hnsw_search_batch_filtered_device(*d_args))
        check(L.hnsw_search_batch_filtered_device_finish(*d_args, None))

    multi()
    t_first = ms(under_set)  # the set's first call: the whole copy, the counts, the compactions
    device()
    t = {"multi": [], "set": [], "device": []}
    for _ in range(REPS):
        for name, fn in (("multi", multi), ("set", under_set), ("device", device)):
            t[name].append(ms(fn))
    identical = bool(a_out.same(b_out))
    # the device form against the set with every row on the graph path
    idx.set_option("filter_exact_max", -1)
    under_set()
    idx.set_option("filter_exact_max", 65536)
    dev_identical = bool(np.array_equal(d_ids.cpu().numpy().view(np.uint32), b_out.ids)
                         and np.array_equal(d_d.cpu().numpy().view(np.uint32), b_out.dists.view(np.uint32))
                         and np.array_equal(d_c.cpu().numpy().view(np.uint32), b_out.counts)
                         and np.array_equal(d_s.cpu().numpy(), b_out.stats))
    # a 1000-id update of row 0 and the call after it
    ids = np.random.default_rng(G).choice(N, 1000, replace=False).astype(np.uint32)
    t_update = ms(lambda: check(L.hnsw_mask_set_update(s, 0, ids.ctypes.data_as(u32p), 1000, 1)))
    t_after = ms(under_set)
    L.hnsw_mask_set_free(s)
    out = dict(paths={str(k): int((a_out.paths == k).sum()) for k in (0, 1, 2)}, identical=identical,
               device_identical_to_set_graph_only=dev_identical, create_ms=t_create, first_call_ms=t_first,
               update_1000_ms=t_update, call_after_update_ms=t_after)
    for name, v in t.items():
        out[name + "_ms"] = float(np.median(v))
        out[name + "_ms_all"] = v
    return out


def main():
    out_path = sys.argv[1]
    gs = [1, 16] if "--quick" in sys.argv else GS
    res = {"shape": dict(n=N, d=D, batch=B, topn=TOPN, ef=EF, reps=REPS,
                         timing="host ms for 1024 queries: one call of each form (device: enqueue + finish); median of "
                                "reps, the three forms alternating, every call ends in a device synchronise; masks "
                                "packed outside; the set warm"),
           "points": []}
    made = {}
    for kind_name in ("f32", "quant8"):
        t0 = time.time()
        idx = build(H.VEC_F32 if kind_name == "f32" else H.VEC_QUANT8)
        print("%s index built in %.1f s" % (kind_name, time.time() - t0), flush=True)
        qs = np.ascontiguousarray(H.synth_rows(0, 0x5EED0002, 0, B, D, 16))
        for family in ("random", "partition"):
            rng = np.random.default_rng(2025)
            for G in gs:
                if (family, G) not in made:  # (the same masks for both kinds, drawn as filter_multi_probe draws them)
                    made[family, G] = packed(family, G, rng)
                p = dict(kind=kind_name, family=family, G=G, **point(idx, qs, made[family, G], G))
                res["points"].append(p)
                print(json.dumps(p), flush=True)
                with open(out_path, "w") as f:
                    json.dump(res, f, indent=1)
        del idx
    print("wrote", out_path)


if __name__ == "__main__":
    main()
