"""Filtered search under the option "rows_f16" beside the plain f32 index over the SAME rows: two
indexes per shape, both by the on-device build, batch 1024, n = 10, ef' = 128, queries and results resident in HBM (the
_device entry points; a window ends in a device synchronise).  Filters: row 0 of a resident mask set allowing 10 % of the
ids, and a label range allowing 50 %.  The exact path: a set row of 20 000 ids under filter_exact_max, through the
host-pointer call (the device forms never plan the exact path), so its windows include the call's copies.  The two
indexes alternate window by window in one session; the report gives the median queries per second with the spread of
the windows and the snapshot's bytes.

With --f32-only the f16 index is left out: the same probe of the f32 filtered path alone, for a library given by
HNSW_MI355X_LIB beside another one, process by process.

usage: python scripts/filt16_probe.py OUT.json [--quick] [--f32-only]   (GPU)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402

M, EFC, B, K, EF, A_EXACT = 16, 32, 1024, 10, 128, 20_000
SHAPES = [(1_000_000, 768), (4_000_000, 128)]
REPS, CALLS = 7, 10


def main():
    out_path = sys.argv[1]
    shapes = [(100_000, 768), (200_000, 128)] if "--quick" in sys.argv else SHAPES
    names = ("f32",) if "--f32-only" in sys.argv else ("f32", "f16")
    dev = torch.device("cuda:0")
    res = {"settings": dict(m=M, ef_cons=EFC, batch=B, n=K, ef=EF, reps=REPS, calls_per_window=CALLS, exact_ids=A_EXACT,
                            timing="host clock around CALLS calls ending in a device synchronise; the indexes alternate "
                                   "window by window in one session"),
           "shapes": []}
    for n, d in shapes:
        X = H.synth_rows(0, 0x5EED0001, 0, n, d, 16)
        Q = H.synth_rows(0, 0x5EED0002, 0, B, d, 16)
        rng = np.random.default_rng(n + d)
        rows = np.zeros((2, n), dtype=bool)
        rows[0] = rng.random(n) < 0.10
        rows[1, rng.choice(n, A_EXACT, replace=False)] = True
        labels = rng.integers(0, 100, n).astype(np.uint32)
        dQ = torch.from_numpy(Q).to(dev)
        lo, hi = (torch.full((B,), v, dtype=torch.int32, device=dev) for v in (0, 49))
        outs = [torch.zeros(s, dtype=t, device=dev) for s, t in
                (((B, K), torch.int32), ((B, K), torch.float32), ((B,), torch.int32), ((B, 4), torch.int32))]
        tail = tuple(o.data_ptr() for o in outs) + (0,)
        point, idx, sets = dict(n=n, d=d), {}, {}
        for name in names:
            ix = H.HNSW.new(M, EFC, d, H.VEC_F32)
            if name == "f16":
                ix.set_option("rows_f16", 1)
            ix.insert_bulk_device(X, 16, False)
            ix.set_labels(labels)
            ix.upload()
            point[name + "_snapshot_bytes"] = ix.stat("snapshot_bytes")
            idx[name], sets[name] = ix, ix.mask_set(rows)
        one = np.ones(B, dtype=np.int64)

        def run(name, what):
            ix, ms = idx[name], sets[name]
            if what == "set_10pct":
                ix.search_batch_filtered_device(dQ.data_ptr(), B, K, EF, ms, None, *tail)
            elif what == "range_50pct":
                ix.search_batch_filtered_range_device(dQ.data_ptr(), B, K, EF, lo.data_ptr(), hi.data_ptr(), *tail)
            else:
                ix.search_batch_filtered_set(Q, K, EF, ms, one)

        for what in ("set_10pct", "range_50pct", "exact_20000"):
            for name in names:
                idx[name].set_option("filter_exact_max", 1 << 30 if what == "exact_20000" else -1)
                with H.kernel_log() as log:
                    run(name, what)  # warm-up, and the kernels that serve the case
                    torch.cuda.synchronize()
                point["%s_%s_kernels" % (name, what)] = sorted(log)
                if what != "exact_20000":
                    point["%s_%s_mean_n_dist" % (name, what)] = float(outs[3].cpu().numpy()[:, 0].mean())
            times = {name: [] for name in names}
            for _ in range(REPS):
                for name in names:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(CALLS):
                        run(name, what)
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) / CALLS)
            for name, t in times.items():
                point["%s_%s_qps_median" % (name, what)] = B / float(np.median(t))
                point["%s_%s_qps_min_max" % (name, what)] = [B / max(t), B / min(t)]
        res["shapes"].append(point)
        print(json.dumps(point), flush=True)
        del idx, sets, X
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
