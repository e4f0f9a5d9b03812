"""Late-interaction search on the host (include/hnsw_mi355x.h, "late-interaction search"): the numpy restatement
(hnsw_rs_amd.late.late_interaction) against a second, deliberately plain one (tests/late_cases.py) bit for bit, its ties
to the fusion of multi-vector search, and everything hnsw_late_interaction_device and hnsw_search_batch_late decide before
they touch a device -- every argument error with its message, nq == 0, the stat keys, the exported symbols and their
prototypes -- and the registers of the kernel that carries the new form.  None of this needs a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import late_cases as LC
from tests import multi_cases as MC
from tests.util import rand_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
N, D = 700, 12
MAX = 0xFFFFFFFF
f32p, u32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
NEW_SYMBOLS = ("hnsw_late_interaction_device", "hnsw_search_batch_late")
KEYS = ("uploads", "late_calls", "late_launches")
SHAPES = [(1, 1), (1, 16), (2, 7), (3, 11), (4, 16), (32, 2), (32, 8)]


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def small(n=N, kind=H.VEC_QUANT8, seed=1):
    vs = rand_vectors(n, D, seed)
    return H.HNSW.new(8, 32, D, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(n, 8, seed))


def label_columns(seed):
    """label columns over the ids of the synthetic lists: many small documents (0 and UINT32_MAX among them), a column
    shorter than the id span, and none at all"""
    rng = np.random.default_rng(seed)
    many = rng.choice(np.array([0, 1, 2, 3, 5, 8, 13, 1000, MAX], dtype=np.uint32), MC.ID_SPAN + 1)
    return {"many": many, "short": many[:120].copy(), "none": None}


# ---- the restatement against the plain one ----------------------------------------------------------------------------
@pytest.mark.parametrize("T,pool", SHAPES)
def test_late_interaction_is_the_plain_loop_bit_for_bit(T, pool):
    dist = LC.memo(MC.table_dist())
    total = T * pool
    for with_counts in (True, False):
        # the planted queries of the fusion's sweep (statuses, a bad id, a NaN vector), then random ones
        Q, ids, counts, statuses = MC.synthetic(T, pool, with_counts, seed=1000 * T + 10 * pool + with_counts)
        Qr, idr, cr, sr = LC.random_case(T, pool, with_counts, 7 * T + pool, MC.ID_SPAN, n_rows=MC.N_TABLE_ROWS)
        Q, ids, statuses = np.concatenate([Q, Qr]), np.concatenate([ids, idr]), np.concatenate([statuses, sr])
        counts = None if counts is None else np.concatenate([counts, cr])
        for kind, labels in label_columns(T + pool).items():
            for mode in (LC.SUM, LC.SUM_SQ):
                for n_out in sorted({1, min(5, total), min(total, 256)}):
                    what = "T=%d pool=%d counts=%s labels=%s mode=%d n_out=%d" % (T, pool, with_counts, kind, mode, n_out)
                    got = H.late_interaction(Q, mode, ids, counts, statuses, dist, labels, n_out, MC.ID_SPAN)
                    want = LC.naive(Q, mode, ids, counts, statuses, dist, labels, n_out, MC.ID_SPAN)
                    LC.assert_late_equal(got, want, what)
                    assert got[0].shape == got[1].shape == got[2].shape == got[3].shape == (len(Q), n_out)
                    # the planted queries did what they are there for
                    assert got[4][0] == 0 and got[5][0] == 0 and got[6][0] == 0 and (got[0][0] == 0).all()
                    assert got[6][4] == (MC.ERR_NAN_INPUT if T > 1 else MC.ERR_OVERFLOW) and got[6][5] == MC.ERR_OVERFLOW
                    assert got[6][6] == MC.ERR_ARG and got[6][7] == MC.ERR_NAN_INPUT
                    for q in (4, 5, 6, 7):
                        assert got[4][q] == 0 and got[5][q] == 0 and (got[0][q] == 0).all() and np.isposinf(got[1][q]).all()
                        assert (got[2][q] == MAX).all() and (got[3][q] == 0).all()
                    if kind == "none":  # one document, holding every candidate
                        live = got[6] == 0
                        assert (got[5][live] <= 1).all() and (got[4][live] == got[5][live]).all()
                    for q in range(len(Q)):  # distinct labels, in (score, label) order, sizes adding up to at most |C|
                        c = int(got[4][q])
                        s, g = got[1][q, :c], got[0][q, :c].astype(np.int64)
                        assert len(set(g.tolist())) == c and not np.isnan(s).any()
                        assert all(s[a] < s[a + 1] or (s[a] == s[a + 1] and g[a] < g[a + 1]) for a in range(c - 1)), what
                        assert (got[3][q, :c] >= 1).all() and got[3][q, :c].sum() <= total


def explicit_dist(table):
    return lambda q_row, ids: np.array([table[int(q_row[0])][int(i)] for i in ids], dtype=np.float32)


def test_a_small_case_by_hand():
    nan = float("nan")
    # documents: 1 = {5, 9}, 2 = {2}, 3 = {7}; two vectors
    table = {0: {5: 1.0, 9: 0.5, 2: 0.75, 7: nan}, 1: {5: 0.25, 9: 2.0, 2: 0.0, 7: nan}}
    labels = np.zeros(10, dtype=np.uint32)
    labels[[5, 9]], labels[2], labels[7] = 1, 2, 3
    Q = np.array([[[0, 0], [1, 0]]], dtype=np.float32)
    ids = np.array([[[9, 5], [7, 2]]], dtype=np.uint32)
    for fn in (H.late_interaction, LC.naive):
        got = fn(Q, LC.SUM, ids, None, None, explicit_dist(table), labels, 4)
        # document 1: 0.5 + 0.25; document 2: 0.75 + 0; document 3: every distance NaN, both minima stay +inf
        assert got[0][0].tolist() == [1, 2, 3, 0] and got[1][0].tolist() == [0.75, 0.75, np.inf, np.inf]
        assert got[2][0].tolist() == [5, 2, MAX, MAX] and got[3][0].tolist() == [2, 1, 1, 0]
        assert got[4][0] == 3 and got[5][0] == 3 and got[6][0] == 0
        got = fn(Q, LC.SUM_SQ, ids, None, None, explicit_dist(table), labels, 2)
        assert got[0][0].tolist() == [1, 2] and got[1][0].tolist() == [0.25 + 0.0625, 0.5625]


def test_one_vector_and_a_label_per_id_is_the_fusion_with_ids_read_as_labels():
    dist = MC.table_dist()
    labels = np.arange(MC.ID_SPAN + 1, dtype=np.uint32)
    for pool in (1, 16, 64):
        for with_counts in (True, False):
            Q, ids, counts, statuses = MC.synthetic(1, pool, with_counts, seed=pool + with_counts)
            Q[:, :, 0] %= 40  # (the table's rows without NaN: a NaN distance drops a candidate there and leaves +inf here)
            for n_out in MC.n_outs(pool):
                late = H.late_interaction(Q, "sum", ids, counts, statuses, dist, labels, n_out, MC.ID_SPAN)
                fused = H.fuse_lists(Q, None, "sum", ids, counts, statuses, dist, n_out, MC.ID_SPAN)
                # (the fusion pads its ids with UINT32_MAX, the late interaction its labels with 0)
                MC.assert_fused_equal((np.where(np.arange(n_out)[None, :] < late[4][:, None], late[0], MAX), late[1], late[4],
                                       late[5], late[6]), fused, "pool=%d n_out=%d" % (pool, n_out))
                taken = np.arange(n_out)[None, :] < late[4][:, None]
                assert (late[2][taken] == late[0][taken]).all() and (late[3][taken] == 1).all()


def test_the_answer_does_not_depend_on_the_order_or_the_number_of_copies_of_an_entry():
    dist = MC.table_dist()
    rng = np.random.default_rng(5)
    labels = label_columns(3)["many"]
    T, pool = 3, 12
    Q, ids, _, statuses = LC.random_case(T, pool, False, 11, MC.ID_SPAN)
    want = H.late_interaction(Q, "sum_sq", ids, None, statuses, dist, labels, 8, MC.ID_SPAN)
    shuffled = ids.copy()
    for q in range(ids.shape[0]):  # entries permuted inside each list and moved between the lists
        shuffled[q] = rng.permutation(ids[q].reshape(-1)).reshape(T, pool)
    LC.assert_late_equal(H.late_interaction(Q, "sum_sq", shuffled, None, statuses, dist, labels, 8, MC.ID_SPAN), want, "permuted")
    doubled = np.concatenate([ids, ids[:, ::-1, :]], axis=2)  # every list followed by a copy of another one
    LC.assert_late_equal(H.late_interaction(Q, "sum_sq", doubled, None, statuses, dist, labels, 8, MC.ID_SPAN), want, "duplicated")


def test_all_labels_equal_is_one_document_scored_by_the_minima_over_all_candidates():
    dist = MC.table_dist()
    T, pool = 4, 9
    Q, ids, counts, statuses = LC.random_case(T, pool, True, 21, MC.ID_SPAN)
    for labels in (None, np.full(MC.ID_SPAN, 77, dtype=np.uint32)):
        for mode in (LC.SUM, LC.SUM_SQ):
            got = H.late_interaction(Q, mode, ids, counts, statuses, dist, labels, 3, MC.ID_SPAN)
            for q in range(1, Q.shape[0]):
                cand = np.unique(np.concatenate([ids[q, t, :min(int(counts[q, t]), pool)] for t in range(T)]))
                if cand.size == 0:
                    assert got[4][q] == 0 and got[5][q] == 0
                    continue
                s = None
                for t in range(T):
                    m = np.float32(np.min(dist(Q[q, t], cand)))
                    e = np.float32(m * m) if mode == LC.SUM_SQ else m
                    s = e if s is None else np.float32(s + e)
                assert got[4][q] == 1 and got[5][q] == 1 and got[3][q, 0] == cand.size
                assert got[0][q, 0] == (0 if labels is None else 77)
                assert got[1][q, 0].view(np.uint32) == np.float32(s).view(np.uint32)
                assert (got[0][q, 1:] == 0).all() and np.isposinf(got[1][q, 1:]).all() and (got[2][q, 1:] == MAX).all()


def test_late_interaction_refuses_shapes_beyond_the_limits():
    dist = MC.table_dist()
    Q = np.zeros((2, 33, 2), dtype=np.float32)
    ids = np.zeros((2, 33, 4), dtype=np.uint32)
    for a in ((Q, "sum", ids, None, None, dist, None, 1), (Q[:, :4], "sum", ids[:, :4], None, None, dist, None, 17),
              (Q[:, :4], "sum", ids[:, :4], None, None, dist, None, 0), (Q[:, :3], "sum", ids[:, :4], None, None, dist, None, 1),
              (Q[:, :4], "min", ids[:, :4], None, None, dist, None, 1),
              (Q[:, :2], "sum", np.zeros((2, 2, 513), dtype=np.uint32), None, None, dist, None, 1),
              (Q[:, :2], "sum", np.zeros((2, 2, 512), dtype=np.uint32), None, None, dist, None, 257)):
        with pytest.raises(ValueError):
            H.late_interaction(*a)
    got = H.late_interaction(Q[:, :32], "sum_sq", np.zeros((2, 32, 32), dtype=np.uint32), None, None, dist, None, 256)
    assert got[4].tolist() == [1, 1] and got[5].tolist() == [1, 1] and got[3][:, 0].tolist() == [1, 1]


# ---- argument errors: decided before the device is touched -------------------------------------------------------------
def test_primitive_argument_errors_need_no_device():
    index = small()
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()
    fake = C.c_void_p(256)  # never dereferenced: every call below is refused first

    def call(h=index._h, nq=6, T=3, pool=16, n_out=10, mode=0, Q=fake, i_in=fake, c_in=fake, s_in=fake, labels=fake, scores=fake,
             best=fake, sizes=fake, counts=fake, n_docs=fake, stats=fake):
        return L.hnsw_late_interaction_device(h, nq, T, pool, n_out, mode, Q, i_in, c_in, s_in, labels, scores, best, sizes,
                                              counts, n_docs, stats, None)

    assert call(h=None) == _lib.ERR_ARG
    assert b"null handle" in L.hnsw_last_error()
    for kw in (dict(T=0), dict(T=33), dict(T=33, pool=1, n_out=1)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"late interaction: needs 1 <= n_vecs <= 32", kw
    for kw in (dict(pool=0), dict(n_out=0), dict(n_out=49), dict(T=1, pool=4, n_out=5), dict(T=32, pool=33), dict(T=1, pool=1025),
               dict(T=2, pool=512, n_out=257), dict(T=2, pool=0x80000000, n_out=1)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"late interaction: needs n_vecs * pool <= 1024 and 1 <= n_out <= min(n_vecs * pool, 256)", kw
    for mode in (2, 7, 0xFFFFFFFF):
        assert call(mode=mode) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"late interaction: the mode is HNSW_LATE_SUM (0) or HNSW_LATE_SUM_SQ (1)"
    assert call(T=32, pool=32, n_out=256, mode=1, Q=None) == _lib.ERR_ARG  # (within the limits: the pointer is refused)
    assert b"needs the vectors" in L.hnsw_last_error()
    assert call(nq=1 << 31) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"late interaction: at most 2^31 - 1 queries"
    for name in ("Q", "i_in", "labels", "scores"):
        assert call(**{name: None}) == _lib.ERR_ARG, name
        assert L.hnsw_last_error() == b"late interaction: needs the vectors, the candidates' ids and the label and score outputs", name
    assert call(s_in=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"late interaction: the stats output goes with the candidates' stats, both or neither"
    assert call(stats=None) == _lib.ERR_ARG
    assert b"both or neither" in L.hnsw_last_error()
    # nq == 0 is HNSW_OK whatever else is passed (but for the handle) and launches nothing
    assert call(nq=0) == _lib.OK
    assert call(nq=0, T=0, pool=0, n_out=0, mode=9, Q=None, i_in=None, labels=None, scores=None, stats=None) == _lib.OK
    assert call(nq=0, h=None) == _lib.ERR_ARG
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert call(h=empty._h) == _lib.ERR_EMPTY and call(h=empty._h, nq=0) == _lib.OK
    assert {k: index.stat(k) for k in KEYS} == before and index.stat("uploads") == 0


def test_search_argument_errors_need_no_device():
    index = small()
    T = 3
    Q = rand_vectors(6 * T, D, 12).reshape(6, T, D)
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()

    def rc(h=index, Q=Q, nq=6, T=T, mode=0, n=4, pool=20, ef=32, labels="own"):
        o_l = np.full((6, max(n, 1)), 7, dtype=np.uint32) if isinstance(labels, str) else labels
        o_s, o_b = np.full((6, max(n, 1)), 3.5, dtype=np.float32), np.full((6, max(n, 1)), 6, dtype=np.uint32)
        o_z, o_c, o_d = np.full((6, max(n, 1)), 5, dtype=np.uint32), np.full(6, 9, dtype=np.uint32), np.full(6, 8, dtype=np.uint32)
        code = L.hnsw_search_batch_late(None if h is None else h._h, ptr(Q, f32p), nq, T, mode, n, pool, ef, ptr(o_l, u32p),
                                        ptr(o_s, f32p), ptr(o_b, u32p), ptr(o_z, u32p), ptr(o_c, u32p), ptr(o_d, u32p), None)
        if code != _lib.OK:  # an error leaves every output as it was
            assert (o_s == 3.5).all() and (o_b == 6).all() and (o_z == 5).all() and (o_c == 9).all() and (o_d == 8).all()
            assert o_l is None or (o_l == 7).all()
        return code

    assert rc(h=None) == _lib.ERR_ARG
    for kw in (dict(T=0), dict(T=33, pool=4)):
        assert rc(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"late search: needs 1 <= n_vecs <= 32", kw
    for kw in (dict(pool=0), dict(n=0), dict(n=61), dict(pool=342), dict(T=32, pool=33), dict(T=2, pool=512, n=257)):
        assert rc(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"late search: needs n_vecs * pool <= 1024 and 1 <= n <= min(n_vecs * pool, 256)", kw
    assert rc(mode=2) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"late search: the mode is HNSW_LATE_SUM (0) or HNSW_LATE_SUM_SQ (1)"
    assert rc(Q=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"late search: needs queries, a label buffer and at most 2^31 - 1 vectors in all"
    assert rc(labels=None) == _lib.ERR_ARG
    assert rc(nq=(1 << 31) // 3 + 1) == _lib.ERR_ARG
    assert b"2^31 - 1 vectors" in L.hnsw_last_error()
    # nq == 0 is HNSW_OK whatever else is missing (but for the handle)
    assert rc(nq=0) == _lib.OK and rc(nq=0, Q=None, labels=None, pool=0, n=0, T=0, mode=5) == _lib.OK
    assert rc(nq=0, h=None) == _lib.ERR_ARG
    after = {k: index.stat(k) for k in KEYS}
    assert after == before and index.stat("uploads") == 0
    # the candidate call's limit while ids are deleted
    index.mark_deleted(np.array([3, 5]))
    assert rc(pool=65, n=4) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"late search: needs pool <= 64 while ids are deleted"
    assert index.stat("uploads") == 0
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert rc(h=empty) == _lib.ERR_EMPTY


def test_python_wrapper_argument_handling():
    index = small()
    Q = rand_vectors(12, D, 12).reshape(6, 2, D)
    with pytest.raises(H.HnswError) as e:
        index.search_batch_late(Q[:, :, :5], 3, 10, 32)
    assert e.value.code == _lib.ERR_BAD_DIM
    with pytest.raises(H.HnswError) as e:
        index.search_batch_late(Q[:, 0], 3, 10, 32)  # [nq, dim]: not a multi-vector call
    assert e.value.code == _lib.ERR_BAD_DIM
    with pytest.raises(ValueError):
        index.search_batch_late(Q, 3, 10, 32, mode="min")
    with pytest.raises(H.HnswError) as e:  # the library's own refusal, before any device
        index.search_batch_late(Q, 21, 10, 32)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(H.HnswError) as e:
        index.search_batch_late(Q, 3, 513, 32)
    assert e.value.code == _lib.ERR_ARG
    got = index.search_batch_late(Q[:0], 3, 10, 32, mode="sum_sq")  # nq == 0
    assert got[0].shape == got[1].shape == got[2].shape == got[3].shape == (0, 3) and got[4].shape == got[5].shape == (0,)
    with pytest.raises(H.HnswError) as e:
        index.late_interaction_device(4, 2, 10, 21, "sum", 256, 256, None, None, 256, 256)
    assert e.value.code == _lib.ERR_ARG
    index.late_interaction_device(0, 2, 10, 3, "sum_sq", None, None, None, None, None, None)  # nq == 0
    assert index.stat("uploads") == 0


# ---- the stat keys and the ABI ----------------------------------------------------------------------------------------
def test_stat_keys_exist_and_read_zero():
    index = small(n=50)
    for key in ("late_calls", "late_launches"):
        assert index.stat(key) == 0


def c_type_of(decl):
    """a parameter of a prototype -> the ctypes type the binding must use (device pointers d_*, the stream and the handle
    are bound as void pointers)"""
    decl = re.sub(r"/\*.*?\*/", "", decl).strip()
    name = re.search(r"(\w+)$", decl).group(1)
    kind = decl[: -len(name)].replace("const", "").replace(" ", "")
    if name.startswith("d_") or kind in ("void*", "hnsw_index*"):
        assert kind.endswith("*"), decl
        return C.c_void_p
    return {"float*": f32p, "uint32_t*": u32p, "uint8_t*": u8p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32,
            "float": C.c_float, "hnsw_query_stats*": C.POINTER(_lib.QueryStats)}[kind]


def test_symbols_are_exported_and_prototypes_match_the_binding():
    header = open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        m = re.search(r"^int %s\((.*?)\);" % name, header, re.S | re.M)
        assert m, name
        params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int
        assert [c_type_of(p) for p in params] == argtypes, name
    assert len(_lib.SYMBOLS[NEW_SYMBOLS[0]][1]) == 18 and len(_lib.SYMBOLS[NEW_SYMBOLS[1]][1]) == 15
    for define, value in (("HNSW_LATE_MAX_VECS", H.LATE_MAX_VECS), ("HNSW_LATE_MAX_CANDS", H.LATE_MAX_CANDS),
                          ("HNSW_LATE_MAX_DOCS", H.LATE_MAX_DOCS), ("HNSW_LATE_SUM", H.LATE_SUM),
                          ("HNSW_LATE_SUM_SQ", H.LATE_SUM_SQ)):
        assert re.search(r"#define %s %d\b" % (define, value), header), define
    assert (H.LATE_MAX_VECS, H.LATE_MAX_CANDS, H.LATE_MAX_DOCS, H.LATE_SUM, H.LATE_SUM_SQ) == (32, 1024, 256, 0, 1)
    assert "THE LATE INTERACTION" in header
    for method in ("search_batch_late", "late_interaction_device"):
        assert hasattr(H.HNSW, method), method
    assert callable(H.late_interaction)


# ---- the kernel that carries the new form ------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_distance_kernel_carries_the_late_interaction_without_scratch_or_vgpr_spills(tmp_path):
    """exact_scan.hip compiled for gfx950 with the Makefile's flags: the late interaction is a source form of
    hx_distance_kernel, whose two instantiations stay the only ones and run without scratch and without spilled vector
    registers"""
    src = os.path.join(ROOT, "hnsw_rs_amd", "csrc", "exact_scan.hip")
    assert "late_interaction<KIND>" in open(src).read(), "the late interaction is a source form of hx_distance_kernel"
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
           "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "exact_scan.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    seam = {k: v for k, v in kernels.items() if "hx_distance_kernel" in k}
    assert len(seam) == 2 and sum("ILi0E" in k for k in seam) == 1 and sum("ILi1E" in k for k in seam) == 1, sorted(kernels)
    for name, r in seam.items():
        assert "ScratchSize" in r and "VGPRs Spill" in r, (name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        assert r.get("VGPRs", 0) <= 256, (name, r)
