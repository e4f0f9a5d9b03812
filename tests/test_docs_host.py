"""Exact document scoring on the host (include/hnsw_mi355x.h, "exact document scoring"): the numpy restatement
(hnsw_rs_amd.docs.score_documents) against a second, deliberately plain one (tests/docs_cases.py) bit for bit, a case by
hand, its defining tie to the exhaustive Chamfer ranking, and everything hnsw_score_documents_device and
hnsw_search_batch_late_exact decide before they touch a device -- every argument error with its message, nq == 0, the stat
keys, the exported symbols and their prototypes -- and the registers of the kernel that carries the new form.  None of
this needs a GPU."""
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
from tests import docs_cases as DC
from tests import multi_cases as MC
from tests.test_late_host import c_type_of, explicit_dist
from tests.util import rand_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
N, D = 700, 12
MAX = 0xFFFFFFFF
f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
NEW_SYMBOLS = ("hnsw_score_documents_device", "hnsw_search_batch_late_exact")
KEYS = ("uploads", "docs_calls", "docs_launches", "doc_index_uploads", "doc_index_keys_uploaded", "late_launches")
SPAN = MC.ID_SPAN


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def small(n=N, kind=H.VEC_QUANT8, seed=1):
    vs = rand_vectors(n, D, seed)
    return H.HNSW.new(8, 32, D, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(n, 8, seed))


# ---- the restatement against the plain one ----------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3, 32])
@pytest.mark.parametrize("n_in", [1, 63, 64, 65, 256])
def test_score_documents_is_the_plain_loop_bit_for_bit(n_in, T):
    dist = MC.table_dist()
    columns, deleted = DC.host_columns(SPAN, n_in + T)
    for with_counts in (True, False):
        Q, docs_in, counts, statuses = DC.host_lists(T, n_in, with_counts, 1000 * T + 10 * n_in + with_counts)
        for kind, labels in columns.items():
            # the big document (label 13, 100 rows under "few") whole, and every document cut to its 7 lowest ids
            for mode, rows_cap, gone in ((DC.SUM, 4096, deleted), (DC.SUM_SQ, 7, None)):
                for n_out in sorted({1, min(10, n_in), n_in}):
                    what = "T=%d n_in=%d counts=%s labels=%s mode=%d n_out=%d" % (T, n_in, with_counts, kind, mode, n_out)
                    a = (Q, mode, docs_in, counts, statuses, dist, labels, gone, n_out, rows_cap, SPAN)
                    got, want = H.score_documents(*a), DC.naive(*a)
                    DC.assert_late_equal(got, want, what)
                    assert got[0].shape == got[1].shape == got[2].shape == got[3].shape == (DC.NQ, n_out)
                    # the planted lists did what they are there for
                    assert got[4][0] == 0 and got[5][0] == 0 and got[6][0] == 0  # a count of 0 / labels without a row
                    assert got[6][2] == DC.ERR_OVERFLOW and got[6][3] == DC.ERR_NAN_INPUT and (got[6] != 0).sum() == 2
                    for q in (0, 2, 3):
                        assert got[4][q] == 0 and got[5][q] == 0 and (got[0][q] == 0).all() and np.isposinf(got[1][q]).all()
                        assert (got[2][q] == MAX).all() and (got[3][q] == 0).all()
                    if kind == "none":  # one document: label 0, the whole index
                        assert (got[5] <= 1).all() and (got[0] == 0).all()
                        live_rows = SPAN - (0 if gone is None else len(gone))
                        assert (got[3][got[5] == 1, 0] == live_rows).all()
                        assert (got[5][4] == 0) and got[5][1] == (1 if (docs_in[1] == 0).any() else 0)
                    else:
                        # one label n_in times: one document (the big one under "few", cut by rows_cap 7)
                        assert got[5][4] == 1 and got[0][4, 0] == 13 and got[3][4, 0] >= (100 if kind == "few" else 1)
                        # labels without a row are no documents; label 5's rows are all deleted under `gone`
                        assert (labels == 5).any() and got[5][5] == (1 if gone is None and (docs_in[5] == 5).any() else 0), what
                    for q in range(DC.NQ):  # distinct labels, in (score, label) order
                        c = int(got[4][q])
                        s, g = got[1][q, :c], got[0][q, :c].astype(np.int64)
                        assert len(set(g.tolist())) == c and not np.isnan(s).any() and (got[3][q, :c] >= 1).all()
                        assert all(s[k] < s[k + 1] or (s[k] == s[k + 1] and g[k] < g[k + 1]) for k in range(c - 1)), what


def test_a_document_cut_by_rows_cap_is_scored_over_its_lowest_ids_and_reports_its_full_size():
    dist = MC.table_dist()
    labels = np.full(SPAN, 9, dtype=np.uint32)
    labels[::3] = 4  # document 4: ids 0, 3, 6, ...; document 9: the rest
    Q = np.zeros((1, 2, 2), dtype=np.float32)
    Q[0, :, 0] = (3, 17)
    docs_in = np.array([[9, 4, 9]], dtype=np.uint32)
    for fn in (H.score_documents, DC.naive):
        whole = fn(Q, "sum" if fn is H.score_documents else DC.SUM, docs_in, None, None, dist, labels, None, 2, 4096, SPAN)
        cut = fn(Q, "sum" if fn is H.score_documents else DC.SUM, docs_in, None, None, dist, labels, None, 2, 5, SPAN)
        assert whole[5][0] == 2 and cut[5][0] == 2 and sorted(cut[3][0].tolist()) == [100, 200] == sorted(whole[3][0].tolist())
        for k in range(2):  # the cut document: the minima over its five lowest ids
            g = int(cut[0][0, k])
            rows = np.flatnonzero(labels == g)[:5]
            s = np.float32(np.min(dist(Q[0, 0], rows))) + np.float32(np.min(dist(Q[0, 1], rows)))
            assert cut[1][0, k] == np.float32(s) and cut[2][0, k] in rows
        assert (whole[1][0] <= cut[1][0][np.argsort(cut[0][0])][np.argsort(np.argsort(whole[0][0]))]).all()


def test_a_small_case_by_hand():
    nan = float("nan")
    # documents: 1 = {5, 9}, 2 = {2}, 3 = {7}, 0 = the other ids; id 8 (label 2) is deleted; two vectors
    table = {0: {i: 9.0 for i in range(10)}, 1: {i: 9.0 for i in range(10)}}
    table[0].update({5: 1.0, 9: 0.5, 2: 0.75, 7: nan, 8: 0.0})
    table[1].update({5: 0.25, 9: 2.0, 2: 0.0, 7: nan, 8: 0.0})
    labels = np.zeros(10, dtype=np.uint32)
    labels[[5, 9]], labels[[2, 8]], labels[7] = 1, 2, 3
    Q = np.array([[[0, 0], [1, 0]]], dtype=np.float32)
    docs_in = np.array([[3, 2, 1, 2, 6]], dtype=np.uint32)  # (label 6 has no row; label 2 is named twice)
    for fn in (H.score_documents, DC.naive):
        got = fn(Q, DC.SUM, docs_in, None, None, explicit_dist(table), labels, np.array([8]), 5, 4, 10)
        # document 1: 0.5 + 0.25; document 2 without the deleted id 8: 0.75 + 0; document 3: both minima stay +inf
        assert got[0][0].tolist() == [1, 2, 3, 0, 0] and got[1][0].tolist() == [0.75, 0.75, np.inf, np.inf, np.inf]
        assert got[2][0].tolist() == [5, 2, MAX, MAX, MAX] and got[3][0].tolist() == [2, 1, 1, 0, 0]
        assert got[4][0] == 3 and got[5][0] == 3 and got[6][0] == 0
        got = fn(Q, DC.SUM_SQ, docs_in, np.array([3]), None, explicit_dist(table), labels, None, 2, 1, 10)
        # three entries present: 3, 2, 1; rows_cap 1: document 1 is id 5 alone (1 + 0.0625), document 2 id 2 (id 8 is back:
        # size 2, and the lowest id is still 2)
        assert got[0][0].tolist() == [2, 1] and got[1][0].tolist() == [0.5625, 1.0625] and got[3][0].tolist() == [2, 2]
        assert got[2][0].tolist() == [2, 5] and got[5][0] == 3 and got[4][0] == 2


def test_scoring_every_label_whole_is_the_exhaustive_chamfer_ranking():
    """the defining property: every document named, rows_cap at least the largest document -> the ranking computed from
    dist over all live ids, label by label"""
    dist = MC.table_dist()
    rng = np.random.default_rng(8)
    labels = rng.integers(0, 40, SPAN).astype(np.uint32)
    deleted = rng.choice(SPAN, 25, replace=False)
    T = 4
    Q = np.zeros((6, T, 2), dtype=np.float32)
    Q[:, :, 0] = rng.integers(0, 40, (6, T))
    every = np.tile(np.arange(40, dtype=np.uint32), (6, 1))
    got = H.score_documents(Q, "sum", every, None, None, dist, labels, deleted, 40, SPAN, SPAN)
    live = np.setdiff1d(np.arange(SPAN), deleted)
    for q in range(6):
        exhaustive = []
        for g in range(40):
            rows = live[labels[live] == g]
            s = None
            for t in range(T):
                m = np.float32(np.min(dist(Q[q, t], rows)))
                s = m if s is None else np.float32(s + m)
            exhaustive.append((s, g, rows.size))
        exhaustive.sort(key=lambda x: (x[0], x[1]))
        assert got[4][q] == 40 and got[5][q] == 40
        assert got[0][q].tolist() == [g for _, g, _ in exhaustive] and got[3][q].tolist() == [z for _, _, z in exhaustive]
        assert np.array_equal(got[1][q].view(np.uint32), np.array([s for s, _, _ in exhaustive], dtype=np.float32).view(np.uint32))


def test_score_documents_refuses_shapes_beyond_the_limits():
    dist = MC.table_dist()
    Q = np.zeros((2, 33, 2), dtype=np.float32)
    docs = np.zeros((2, 257), dtype=np.uint32)
    for a in ((Q, "sum", docs[:, :4], None, None, dist, None, None, 1, 1, SPAN),
              (Q[:, :4], "sum", docs, None, None, dist, None, None, 1, 1, SPAN),
              (Q[:, :4], "sum", docs[:, :4], None, None, dist, None, None, 5, 1, SPAN),
              (Q[:, :4], "sum", docs[:, :4], None, None, dist, None, None, 0, 1, SPAN),
              (Q[:, :4], "sum", docs[:, :4], None, None, dist, None, None, 1, 0, SPAN),
              (Q[:, :4], "sum", docs[:, :4], None, None, dist, None, None, 1, H.DOCS_MAX_ROWS + 1, SPAN),
              (Q[:, :4], "min", docs[:, :4], None, None, dist, None, None, 1, 1, SPAN),
              (Q[:1, :4], "sum", docs[:, :4], None, None, dist, None, None, 1, 1, SPAN)):
        with pytest.raises(ValueError):
            H.score_documents(*a)
    got = H.score_documents(Q[:, :32], "sum_sq", docs[:, :256], None, None, dist, None, None, 256, H.DOCS_MAX_ROWS, SPAN)
    assert got[4].tolist() == [1, 1] and got[5].tolist() == [1, 1] and got[3][:, 0].tolist() == [SPAN, SPAN]


# ---- argument errors: decided before the device is touched -------------------------------------------------------------
def test_primitive_argument_errors_need_no_device():
    index = small()
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()
    fake = C.c_void_p(256)  # never dereferenced: every call below is refused first

    def call(h=index._h, nq=6, T=3, n_in=16, n_out=10, rows_cap=64, mode=0, Q=fake, docs=fake, c_in=fake, s_in=fake, labels=fake,
             scores=fake, best=fake, sizes=fake, counts=fake, n_docs=fake, stats=fake):
        return L.hnsw_score_documents_device(h, nq, T, n_in, n_out, rows_cap, mode, Q, docs, c_in, s_in, labels, scores, best,
                                             sizes, counts, n_docs, stats, None)

    assert call(h=None) == _lib.ERR_ARG
    assert b"null handle" in L.hnsw_last_error()
    for kw in (dict(T=0), dict(T=33), dict(T=33, n_in=0)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"document scoring: needs 1 <= n_vecs <= 32", kw
    for kw in (dict(n_in=0), dict(n_out=0), dict(n_out=17), dict(n_in=257, n_out=1), dict(rows_cap=0), dict(rows_cap=1048577),
               dict(rows_cap=0xFFFFFFFF), dict(n_in=0x80000000, n_out=1)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"document scoring: needs 1 <= n_out <= n_in <= 256 and 1 <= rows_cap <= 1048576", kw
    for mode in (2, 7, 0xFFFFFFFF):
        assert call(mode=mode) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"document scoring: the mode is HNSW_LATE_SUM (0) or HNSW_LATE_SUM_SQ (1)"
    assert call(nq=1 << 31) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"document scoring: at most 2^31 - 1 queries"
    for name in ("Q", "docs", "labels", "scores"):
        assert call(T=32, n_in=256, n_out=256, rows_cap=1048576, mode=1, **{name: None}) == _lib.ERR_ARG, name  # (within the limits)
        assert L.hnsw_last_error() == b"document scoring: needs the vectors, the documents' labels and the label and score outputs", name
    assert call(s_in=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"document scoring: the stats output goes with the documents' stats, both or neither"
    assert call(stats=None) == _lib.ERR_ARG
    assert b"both or neither" in L.hnsw_last_error()
    # nq == 0 is HNSW_OK whatever else is passed (but for the handle) and launches nothing
    assert call(nq=0) == _lib.OK
    assert call(nq=0, T=0, n_in=0, n_out=0, rows_cap=0, mode=9, Q=None, docs=None, labels=None, scores=None, stats=None) == _lib.OK
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

    def rc(h=index, Q=Q, nq=6, T=T, mode=0, n=4, n_cand=8, rows_cap=64, pool=20, ef=32, labels="own"):
        o_l = np.full((6, max(n, 1)), 7, dtype=np.uint32) if isinstance(labels, str) else labels
        o_s, o_b = np.full((6, max(n, 1)), 3.5, dtype=np.float32), np.full((6, max(n, 1)), 6, dtype=np.uint32)
        o_z, o_c, o_d = np.full((6, max(n, 1)), 5, dtype=np.uint32), np.full(6, 9, dtype=np.uint32), np.full(6, 8, dtype=np.uint32)
        code = L.hnsw_search_batch_late_exact(None if h is None else h._h, ptr(Q, f32p), nq, T, mode, n, n_cand, rows_cap, pool, ef,
                                              ptr(o_l, u32p), ptr(o_s, f32p), ptr(o_b, u32p), ptr(o_z, u32p), ptr(o_c, u32p),
                                              ptr(o_d, u32p), None)
        if code != _lib.OK:  # an error leaves every output as it was
            assert (o_s == 3.5).all() and (o_b == 6).all() and (o_z == 5).all() and (o_c == 9).all() and (o_d == 8).all()
            assert o_l is None or (o_l == 7).all()
        return code

    assert rc(h=None) == _lib.ERR_ARG
    for kw in (dict(T=0), dict(T=33, pool=4)):
        assert rc(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"exact late search: needs 1 <= n_vecs <= 32", kw
    shape = (b"exact late search: needs n_vecs * pool <= 1024, 1 <= n <= n_cand <= min(n_vecs * pool, 256) and "
             b"1 <= rows_cap <= 1048576")
    for kw in (dict(pool=0), dict(n=0), dict(n=9), dict(n_cand=61), dict(pool=342), dict(T=32, pool=33), dict(T=2, pool=512, n_cand=257),
               dict(rows_cap=0), dict(rows_cap=1048577), dict(n=1, n_cand=0)):
        assert rc(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == shape, kw
    assert rc(mode=2) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"exact late search: the mode is HNSW_LATE_SUM (0) or HNSW_LATE_SUM_SQ (1)"
    assert rc(Q=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"exact late search: needs queries, a label buffer and at most 2^31 - 1 vectors in all"
    assert rc(labels=None) == _lib.ERR_ARG
    assert rc(nq=(1 << 31) // 3 + 1) == _lib.ERR_ARG
    assert b"2^31 - 1 vectors" in L.hnsw_last_error()
    # nq == 0 is HNSW_OK whatever else is missing (but for the handle)
    assert rc(nq=0) == _lib.OK and rc(nq=0, Q=None, labels=None, pool=0, n=0, n_cand=0, rows_cap=0, T=0, mode=5) == _lib.OK
    assert rc(nq=0, h=None) == _lib.ERR_ARG
    assert {k: index.stat(k) for k in KEYS} == before and index.stat("uploads") == 0
    # the candidate call's limit while ids are deleted
    index.mark_deleted(np.array([3, 5]))
    assert rc(pool=65) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"exact late search: needs pool <= 64 while ids are deleted"
    assert index.stat("uploads") == 0
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert rc(h=empty) == _lib.ERR_EMPTY


def test_python_wrapper_argument_handling():
    index = small()
    Q = rand_vectors(12, D, 12).reshape(6, 2, D)
    with pytest.raises(H.HnswError) as e:
        index.search_batch_late_exact(Q[:, :, :5], 3, 6, 10, 32)
    assert e.value.code == _lib.ERR_BAD_DIM
    with pytest.raises(ValueError):
        index.search_batch_late_exact(Q, 3, 6, 10, 32, mode="min")
    with pytest.raises(H.HnswError) as e:  # the library's own refusal, before any device
        index.search_batch_late_exact(Q, 7, 6, 10, 32)
    assert e.value.code == _lib.ERR_ARG
    got = index.search_batch_late_exact(Q[:0], 3, 6, 10, 32, mode="sum_sq", rows_cap=5)  # nq == 0
    assert got[0].shape == got[1].shape == got[2].shape == got[3].shape == (0, 3) and got[4].shape == got[5].shape == (0,)
    with pytest.raises(H.HnswError) as e:
        index.score_documents_device(4, 2, 10, 21, 64, "sum", 256, 256, None, None, 256, 256)
    assert e.value.code == _lib.ERR_ARG
    index.score_documents_device(0, 2, 10, 3, 64, "sum_sq", None, None, None, None, None, None)  # nq == 0
    assert index.stat("uploads") == 0


# ---- the stat keys and the ABI ----------------------------------------------------------------------------------------
def test_stat_keys_exist_and_read_zero():
    index = small(n=50)
    for key in ("docs_calls", "docs_launches", "doc_index_uploads", "doc_index_keys_uploaded"):
        assert index.stat(key) == 0


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
    assert len(_lib.SYMBOLS[NEW_SYMBOLS[0]][1]) == 19 and len(_lib.SYMBOLS[NEW_SYMBOLS[1]][1]) == 17
    for define, value in (("HNSW_DOCS_MAX_IN", H.DOCS_MAX_IN), ("HNSW_DOCS_MAX_ROWS", H.DOCS_MAX_ROWS)):
        assert re.search(r"#define %s %d\b" % (define, value), header), define
    assert H.DOCS_MAX_IN == 256 and H.DOCS_MAX_ROWS >= 4096
    assert "THE DOCUMENT SCORING" in header
    for method in ("search_batch_late_exact", "score_documents_device"):
        assert hasattr(H.HNSW, method), method
    assert callable(H.score_documents)


# ---- the kernel that carries the new form ------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_distance_kernel_carries_the_document_scoring_without_scratch_or_vgpr_spills(tmp_path):
    """exact_scan.hip compiled for gfx950 with the Makefile's flags: the document scoring is a source form of
    hx_distance_kernel that shares the late interaction's pass loop -- ONE call site of the row distance in it -- whose two
    instantiations stay the only ones and run without scratch and without spilled vector registers"""
    src = os.path.join(ROOT, "hnsw_rs_amd", "csrc", "exact_scan.hip")
    text = open(src).read()
    assert "dv.docs" in text and text.count("late_interaction<KIND>(") == 1, "the scoring is late_interaction's other half"
    body = text[text.index("void late_interaction("):text.index("The kernel's sixth form")]
    assert body.count("dist_any_dim<KIND>(") == 1 and "d.doc_keys" in body
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
