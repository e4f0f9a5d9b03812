"""hnsw_brute_force_fast under the option "rows_f16" beside the plain f32 index over the SAME widened rows (DESIGN.md
section 38): wall time of the call on both, alternated, warm; which kernels answered; and at gauss(5000, 128, 14), where
few queries are safe at 4 E, the share of queries identical to the exact answer.  Rows: H.synth_rows widened, with the
binary16 subnormals set to zero (`screened`) so that the screen answers, and as drawn (the exact path answers).

usage: python scripts/truth16_probe.py OUT.json [--quick | --trace]   (GPU)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hnsw_rs_amd as H  # noqa: E402
from tests import ground_truth_inputs as G  # noqa: E402


def flat(X, f16):
    N, d = X.shape
    idx = H.HNSW.new(8, 16, d, H.VEC_F32)
    if f16:
        idx.set_option("rows_f16", 1)
    idx.import_points(X, np.zeros(N, dtype=np.uint8))
    idx.import_layer(0, np.arange(N, dtype=np.uint32), np.zeros(N + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    idx.set_ep(0)
    idx.upload()
    return idx


def timed(idx, Q, k, reps):
    idx.brute_force_fast(Q, k)
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        idx.brute_force_fast(Q, k)
        out.append(time.perf_counter() - t)
    return out


def shape(N, d, nq, reps, screened):
    X = H.synth_rows(0, 0x5EED0001, 0, N, d).astype(np.float16).astype(np.float32)
    Q = H.synth_rows(0, 0x5EED0002, 0, nq, d)
    tiny = (X != 0) & (np.abs(X) < 2.0 ** -14)
    if screened:
        X[tiny] = 0
    a, b = flat(X, True), flat(X, False)
    with H.kernel_log() as log:
        got = a.brute_force_fast(Q, 10)
    want = b.brute_force_fast(Q, 10)
    t16, t32 = [], []
    for _ in range(reps):  # alternated
        t16 += timed(a, Q, 10, 1)
        t32 += timed(b, Q, 10, 1)
    r = {"N": N, "d": d, "nq": nq, "screened": screened, "subnormal_elements": int(tiny.sum()), "kernels": sorted(log),
         "same_ids_as_f32_fast": float((got[0] == want[0]).all(axis=1).mean()),
         "f16_s": t16, "f32_s": t32, "ratio_f32_over_f16": float(np.median(t32) / np.median(t16)),
         "flop_2Ndnq": 2.0 * N * d * nq}
    print(json.dumps(r), flush=True)
    return r


def main():
    out, quick, trace = sys.argv[1], "--quick" in sys.argv, "--trace" in sys.argv
    res = []
    for N, d, nq in ([(100000, 128, 256)] if quick else [(1000000, 128, 2048), (250000, 768, 256)]):
        for screened in ((True,) if trace else (True, False)):
            res.append(shape(N, d, nq, 1 if trace else 3 if quick else 5, screened))
    if trace:  # (under rocprofv3 --kernel-trace --stats: the screened shapes once, for the kernels' own durations)
        return
    X, Q = G.gauss(5000, 128, 14)
    X = X.astype(np.float16).astype(np.float32)
    X[np.abs(X) < 2.0 ** -14] = 0
    want = flat(X, False).brute_force(Q, G.K)
    got = flat(X, True).brute_force_fast(Q, G.K)
    m = G.margin(X, Q, G.K, want[0])
    res.append({"gauss": [5000, 128, 14], "safe_share_at_4E": float((m > 4).mean()), "safe_share_at_1E": float((m > 1).mean()),
                "identical_share": float(((got[0] == want[0]).all(axis=1) & (got[1].view(np.uint32) == want[1].view(np.uint32)).all(axis=1)).mean())})
    print(json.dumps(res[-1]), flush=True)
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
