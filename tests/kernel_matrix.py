"""The search-side kernel matrix: one row per case, each naming the kernel instantiation(s) a call must launch, and
the runner that holds the call to the CPU oracle (or, filtered, to tests/filtered_restate.py).

tests/test_gpu_kernel_matrix.py runs the rows on an MI355X (the rows of an environment group in a child process of
their own, `python -m tests.kernel_matrix <group>`: the switches are read once per process).
tests/test_kernel_matrix_complete.py checks, without a GPU, that every instantiation compiled into the library is
named by a row here, by a case of tests/test_gpu_build_restatement.py, or in its own lists with a reason.

A row names the instantiation(s) it pins -- every instantiation is named by one row -- and the calls that must launch
them.  A call gives the vector kind, dimension d, m, inline rows (the "inline_rows" option), entry point, ef, n (the
second run; every call also runs with n = 10), number of queries and environment group.  Entry points: "batch" (search_batch), "layer" (search_layer on layer 0 from `ent`
entries), "device" (search_batch_device + _finish), "distance" (distance_batch), "brute" (brute_force),
"brute_fast" (brute_force_fast), "filtered" (search_batch_filtered on the graph path) and "filtered_exact" (its
exact path).
"""
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

Q8, F32 = 0, 1  # HNSW_VEC_QUANT8, HNSW_VEC_F32 (the KIND template argument)
N_POINTS = 1500
N_QUERIES = 24
MANY = 1100  # queries of a launch with more than 4 waves per CU on MI355X's 256 CUs

GROUPS = {
    "default": {},
    "pair": {"HNSW_MI355X_PAIR": "1"},
    # the LDS level of the two-level visited set closes after 300 ids: every wide search goes on in the HBM level
    "visited2l": {"HNSW_MI355X_VISITED_2L_LIMIT": "300"},
}

# One call of a row: the index (kind, d, m, inline rows), the entry point, ef, the second n, the queries, the
# environment group, the search_layer entries, `also` (instantiations the call launches that another row holds to
# the reference) and `may` (ones it may launch besides: the re-run of queries a first launch gave up).
Call = namedtuple("Call", "kind d m inline entry ef n nq group ent also may")
# A row: the instantiation(s) it pins and the calls that must launch them.  Every instantiation is named by one row.
Row = namedtuple("Row", "kernels calls")
_ROWS = {}


def case(kernels, kind, d, m, inline, entry, ef, n=None, nq=N_QUERIES, group="default", ent=0, also=(), may=()):
    kernels = (kernels,) if isinstance(kernels, str) else tuple(kernels)
    call = Call(kind, d, m, inline, entry, ef, ef if n is None else n, nq, group, ent, tuple(also), tuple(may))
    _ROWS.setdefault(kernels, []).append(call)


def S(kind, p, ds, r, fat=False):
    return "hx_search_kernel<%d, %d, %d, %d, %s>" % (kind, p, ds, r, "true" if fat else "false")


EF_R = {1: 10, 2: 100, 4: 200, 8: 300, 16: 600}  # an ef of each list width (ef <= 64 * R)
# the top registers: ef and n above 64 (R - 1) + 1 (7 / 15 registers full, the last one read out)
EF_TOP = {8: 500, 16: 1000}
# 8-bit any-dimension rows by half-row width P (16-byte pieces): d = 8, 40, 72, 104, 136
D_OF_P = {1: 8, 2: 40, 3: 72, 4: 104, 5: 136}


def compact(kind, p, ds, r, d, m):
    """a compact-layout hx_search_kernel form: its band's ef, and for eight / sixteen registers also the top of the list
    (a 2^14- / 2^15-slot table: LDS level + HBM level) with and without an early switch to the HBM level"""
    case(S(kind, p, ds, r), kind, d, m, 0, "batch", EF_R[r])
    if r in EF_TOP:
        case(S(kind, p, ds, r), kind, d, m, 0, "batch", EF_TOP[r])
        case(S(kind, p, ds, r), kind, d, m, 0, "batch", EF_TOP[r], group="visited2l")


# ---- hx_search_kernel: the compile-time dimensions, compact layout (m = 24: 64-slot rows, where the lean kernels
# step aside; d = 256 / 768 and the any-dimension rows at m = 16)
for kind, p, ds, m in ((Q8, 4, 100, 24), (Q8, 5, 128, 16), (Q8, 9, 256, 16), (Q8, 25, 768, 16),
                       (F32, 25, 100, 24), (F32, 32, 128, 24), (F32, 64, 256, 16), (F32, 192, 768, 16)):
    for r in (1, 2, 4, 8):
        compact(kind, p, ds, r, ds, m)
for kind, d in ((Q8, 200), (F32, 60)):
    for r in (1, 2, 4, 8, 16):
        compact(kind, 0, 0, r, d, 16)
# the any-dimension 8-bit rows, compact layout, P = 1 .. 5
for p, d in D_OF_P.items():
    for r in (1, 2, 4, 8):
        compact(Q8, p, 0, r, d, 16)
# inline rows (FAT): the descent at one and two list registers; at four only P <= 2 and at eight (ef <= 320:
# a 2^13-slot table) only P = 1 fit the block images into 40 KiB -- the others fall back to the compact loop
for p, d in list(D_OF_P.items()) + [(5, 128)]:
    ds = 128 if d == 128 else 0
    case(S(Q8, p, ds, 1, True), Q8, d, 16, 1, "batch", 10)
    case(S(Q8, p, ds, 2, True), Q8, d, 16, 1, "batch", 100)
    case(S(Q8, p, ds, 4, p <= 2), Q8, d, 16, 1, "batch", 200)
    case(S(Q8, p, ds, 8, p <= 1), Q8, d, 16, 1, "batch", 300)
    # ... and at eight registers from ef 321 the table alone is 64 KiB: compact for every P
    case(S(Q8, p, ds, 8), Q8, d, 16, 1, "batch", 400, n=10)
# the search_layer seam (entries <= ef, the host refuses more): d = 100 8-bit inline rows at one and two registers,
# f32 d = 100 / 128 (the lean kernels serve only the whole descent)
case(S(Q8, 4, 100, 1, True), Q8, 100, 16, 1, "layer", 10, ent=3)
case(S(Q8, 4, 100, 2, True), Q8, 100, 16, 1, "layer", 100, ent=3)
case(S(F32, 25, 100, 2), F32, 100, 16, 0, "layer", 100, ent=3)
case(S(F32, 32, 128, 4), F32, 128, 16, 0, "layer", 200, ent=3)
# ef above the register lists: list and visited table in HBM
case("hx_search_spill_kernel<0>", Q8, 200, 16, 0, "batch", 1100, n=1100)
case("hx_search_spill_kernel<1>", F32, 60, 16, 0, "batch", 1100, n=1100)
# the device-pointer entry + _finish (nothing overflows these indexes: _finish launches nothing more)
case(S(F32, 0, 0, 2), F32, 60, 16, 0, "device", 100)
case("hx_lean_q8_kernel<Lst<1> >", Q8, 100, 16, 0, "device", 10)

# ---- lean kernels: the whole ann_by_vector descent at d = 100 (both kinds) and f32 d = 128, S0 = 32; from six
# registers on (ef > 320) with the two-level visited set, also with an early switch to the HBM level
LEAN_EF = (("Lst<1>", 10), ("LstHT", 100), ("Lst<4>", 200), ("Lst<5>", 300), ("Lst<6>", 350), ("Lst<7>", 400),
           ("Lst<8>", 500))
for lst, ef in LEAN_EF:
    for name, kind in (("hx_lean_q8_kernel<%s>" % (lst + " " if lst.endswith(">") else lst), Q8),
                       ("hx_lean_f32_kernel<100, %s, 4>" % lst, F32)):
        case(name, kind, 100, 16, 0, "batch", ef)
        if ef > 320:
            case(name, kind, 100, 16, 0, "batch", ef, group="visited2l")
# f32 d = 128: four-stage gather while a launch leaves each SIMD at most one wave, two-stage beyond
for lst, ef, ck, nq in (("Lst<1>", 10, 4, N_QUERIES), ("LstHT", 100, 4, N_QUERIES), ("Lst<1>", 10, 2, MANY),
                        ("LstHT", 100, 2, MANY), ("Lst<4>", 200, 2, N_QUERIES), ("Lst<6>", 384, 2, N_QUERIES),
                        ("Lst<8>", 500, 2, N_QUERIES)):
    case("hx_lean_f32_kernel<128, %s, %d>" % (lst, ck), F32, 128, 16, 0, "batch", ef, nq=nq)
    if ef > 320:
        case("hx_lean_f32_kernel<128, %s, %d>" % (lst, ck), F32, 128, 16, 0, "batch", ef, group="visited2l")

# ---- opt-in forms (environment groups)
# (a query the two-wave pair gives up -- HNSW_ERR_OVERFLOW, pair_kernel.inc -- runs again on the one-wave kernel)
case("hx_pair_f32_kernel<100, Lst<1> >", F32, 100, 16, 0, "batch", 10, group="pair",
     may=["hx_lean_f32_kernel<100, Lst<1>, 4>"])
case("hx_pair_f32_kernel<100, LstHT>", F32, 100, 16, 0, "batch", 100, group="pair",
     may=["hx_lean_f32_kernel<100, LstHT, 4>"])

# ---- filtered search: the graph kernel at one, two and four list registers per (kind, dimension) form; the exact
# path's compaction, scan and merge
for kind, d, form in ((Q8, 100, "0, 4, 100"), (Q8, 40, "0, 0, 0"), (F32, 100, "1, 25, 100"), (F32, 128, "1, 32, 128"),
                      (F32, 60, "1, 0, 0")):
    for r in (1, 2, 4):
        case("hx_filt_graph_kernel<%s, %d>" % (form, r), kind, d, 16, 0, "filtered", EF_R[r], n=min(EF_R[r], 64), nq=8)
case(("hx_filt_compact_kernel", "hx_filt_scan_kernel<0>", "hx_filt_merge_kernel"), Q8, 40, 16, 0, "filtered_exact", 64,
     nq=8)
case("hx_filt_scan_kernel<1>", F32, 60, 16, 0, "filtered_exact", 64, nq=8,
     also=("hx_filt_compact_kernel", "hx_filt_merge_kernel"))

# ---- distances and brute force
for kind, d in ((Q8, 40), (F32, 60)):
    case("hx_distance_kernel<%d>" % kind, kind, d, 16, 0, "distance", 0, nq=4)
    case("hx_brute_kernel<%d>" % kind, kind, d, 16, 0, "brute", 64)
case(("hx_row_norms_kernel", "hx_brute_mfma_kernel", "hx_pair_distance_kernel"), F32, 60, 16, 0, "brute_fast",
     12)  # (k <= 12)

CASES = [Row(k, tuple(calls)) for k, calls in _ROWS.items()]


def call_id(c):
    return "%s-d%d-m%d-%s%s-ef%d-n%d-q%d%s%s" % ("q8" if c.kind == Q8 else "f32", c.d, c.m, c.entry,
                                                 "-inline" if c.inline else "", c.ef, c.n, c.nq,
                                                 "-ent%d" % c.ent if c.ent else "",
                                                 "" if c.group == "default" else "-" + c.group)


def case_id(row):
    return "+".join(k.replace(" ", "") for k in row.kernels)


# ------------------------------------------------------------------------------------------------------------------
# the runner (imports the product lazily: the completeness test reads the table without a GPU)

def edge_queries(vs, kind):
    """stored rows (distance 0, ties at the head of the list), a constant row (8-bit: quantisation delta 0), rows plus
    a large common offset and, f32, a row whose every distance is +inf (ordered by id)"""
    d = vs.shape[1]
    out = [vs[3], vs[777], np.full(d, 0.25, np.float32), vs[5] + np.float32(1e4), vs[11] - np.float32(1e4)]
    if kind == F32:
        out.append(np.full(d, 1e20, np.float32))
    return np.stack(out).astype(np.float32)


_INDEXES = {}


def fixture(kind, d, m):
    """(index, oracle, vectors) of N_POINTS host-built points, shared by every case of (kind, d, m)"""
    import hnsw_rs_amd as H
    from oracle import oracle_py as O
    from tests.util import oracle_from_product
    key = (kind, d, m)
    if key not in _INDEXES:
        vs = H.synth_rows(0, 0x3A7F0000 + d * 256 + m, 0, N_POINTS, d)
        lv = O.draw_levels(N_POINTS, m, 0x3A7F + d)
        idx = H.HNSW.new(m, 32, d, kind).insert_bulk(vs, 8, False, levels=lv)
        _INDEXES[key] = (idx, oracle_from_product(idx, vs, lv), vs)
    return _INDEXES[key]


def queries(c, vs):
    import hnsw_rs_amd as H
    base = H.synth_rows(0, 0x3A7F9999 + c.d, 0, c.nq, c.d)
    return np.concatenate([base, edge_queries(vs, c.kind)]).astype(np.float32)


def _calls(c, idx, orc, vs, Q, n):
    """-> (run the product, check it against the reference) for one case and one n"""
    import hnsw_rs_amd as H
    from tests.util import assert_search_equal
    what = "%s n=%d" % (call_id(c), n)
    n_points = vs.shape[0]  # (N_POINTS for the matrix's own fixtures)
    if c.entry == "batch":
        out = {}
        return (lambda: out.setdefault("r", idx.search_batch(Q, n, c.ef)),
                lambda: assert_search_equal(out["r"], orc.search_batch(Q, n, c.ef, nthreads=8), what))
    if c.entry == "layer":
        ent = np.arange(c.ent, dtype=np.uint32) * 3 % n_points
        qs = Q[-8:]  # a few queries, the edge ones among them: every call is one launch
        out = []

        def check():
            for q, (g_ids, g_d, g_s) in zip(qs, out):
                w_ids, w_d, w_s = orc.search_layer(0, q, ent, c.ef)
                assert np.array_equal(g_ids, w_ids), (what, g_ids[:8], w_ids[:8])
                assert np.array_equal(g_d.view(np.uint32), w_d.view(np.uint32)), what
                assert tuple(int(x) for x in g_s) == tuple(int(x) for x in w_s), (what, g_s, w_s)
        return (lambda: out.extend(idx.search_layer(0, q, ent, c.ef) for q in qs)), check
    if c.entry == "device":
        import torch
        dev = torch.device("cuda:0")
        nq = Q.shape[0]
        dQ = torch.from_numpy(Q).to(dev)
        d_ids = torch.empty((nq, n), dtype=torch.int32, device=dev)
        d_d = torch.empty((nq, n), dtype=torch.float32, device=dev)
        d_c = torch.empty(nq, dtype=torch.int32, device=dev)
        d_s = torch.empty((nq, 4), dtype=torch.int32, device=dev)
        ptrs = (dQ.data_ptr(), nq, n, c.ef, d_ids.data_ptr(), d_d.data_ptr(), d_c.data_ptr(), d_s.data_ptr(), 0)

        def run():
            idx.search_batch_device(*ptrs)
            idx.search_batch_device_finish(*ptrs)

        def check():
            got = (d_ids.cpu().numpy().view(np.uint32), d_d.cpu().numpy(), d_c.cpu().numpy().view(np.uint32),
                   d_s.cpu().numpy())
            assert (got[3][:, 3] == 0).all(), what
            assert_search_equal(got, orc.search_batch(Q, n, c.ef, nthreads=8), what)
        return run, check
    if c.entry == "distance":
        ids = (np.arange(n_points, dtype=np.uint32)[::-1] * 7 % n_points).astype(np.uint32)
        out = []

        def check():
            for q, got in zip(Q, out):
                want = orc.distance_batch(q, ids)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what
        return (lambda: out.extend(idx.distance_batch(q, ids) for q in Q)), check
    if c.entry in ("brute", "brute_fast"):
        out = {}
        fn = idx.brute_force if c.entry == "brute" else idx.brute_force_fast
        # brute_force_fast screens on the matrix cores (not bit-exact by construction, include/hnsw_mi355x.h): it is
        # held to the exact answer on the base queries, whose neighbours its k + 8 re-rank keeps
        QQ = Q if c.entry == "brute" else Q[:c.nq]

        def check():
            w_ids, w_d = orc.brute_force(QQ, n, nthreads=8)
            g_ids, g_d = out["r"]
            assert np.array_equal(g_ids, w_ids), what
            assert np.array_equal(g_d.view(np.uint32), w_d.view(np.uint32)), what
        return (lambda: out.setdefault("r", fn(QQ, n))), check
    if c.entry in ("filtered", "filtered_exact"):
        from tests.test_gpu_filtered import check as fcheck, restated
        rng = np.random.default_rng(c.d * 31 + c.ef)
        allow = rng.random(n_points) < 0.5
        exact_max = 10 ** 9 if c.entry == "filtered_exact" else -1
        ridx = restated(idx, vs)
        return (lambda: fcheck(idx, ridx, Q, n, c.ef, allow, exact_max=exact_max, what=what)), (lambda: None)
    raise ValueError(c.entry)


def run_call(kernels, c, on=None):
    """run one call of a row: the kernel log must hold exactly the row's instantiations (+ the call's `also`, + any of
    its `may`), the answers must be the reference's.  on: (index, oracle, vectors, queries) to run the call on instead
    of the row's own fixture and queries (tests/numeric_range.py)"""
    import hnsw_rs_amd as H
    idx, orc, vs = on[:3] if on else fixture(c.kind, c.d, c.m)
    idx.set_option("inline_rows", c.inline)
    Q = on[3] if on else queries(c, vs)
    want = set(kernels) | set(c.also)
    for n in sorted({10, c.n}) if c.entry != "distance" else (0,):
        run, check = _calls(c, idx, orc, vs, Q, n)
        run()  # (the first call after an option change uploads the snapshot)
        run, check = _calls(c, idx, orc, vs, Q, n)
        with H.kernel_log() as log:
            run()
        assert want <= set(log) <= want | set(c.may), "%s %s n=%d launched %s" % (
            "+".join(kernels), call_id(c), n, dict(log))
        check()


def run_case(row, group="default"):
    """every call of a row that belongs to `group`"""
    for c in row.calls:
        if c.group == group:
            run_call(row.kernels, c)


def main(group):
    env = GROUPS[group]
    for k, v in env.items():
        assert os.environ.get(k) == v, "run group %s with %s=%s" % (group, k, v)
    calls = 0
    for row in CASES:
        run_case(row, group)
        calls += sum(c.group == group for c in row.calls)
    print("KERNEL MATRIX OK %s %d" % (group, calls))


if __name__ == "__main__":
    main(sys.argv[1])
