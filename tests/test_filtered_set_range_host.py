"""hnsw_search_batch_filtered_set_range, _device and _device_finish on the host (include/hnsw_mi355x.h, "a label range
AND a row of a resident mask set"): everything the three entry points decide before they touch a device -- every
argument error, leaving the outputs untouched, nq == 0 and n == 0 -- the C prototypes against the ctypes binding, the
Python wrapper's argument handling, and the compiled filtered kernels' occupancy against the values they had before the
graph kernel learnt to read a row next to a range.  None of this needs a GPU."""
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
from tests.util import rand_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
N, D = 700, 12
MAX = 0xFFFFFFFF
f32p, u32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
NEW_SYMBOLS = ("hnsw_search_batch_filtered_set_range", "hnsw_search_batch_filtered_set_range_device",
               "hnsw_search_batch_filtered_set_range_device_finish")
KEYS = ("uploads", "label_words_uploaded", "mask_set_words_uploaded", "mask_set_recounts", "filtered_set_range_calls",
        "filtered_set_range_groups", "filtered_set_calls", "filtered_range_calls", "filtered_queries_graph",
        "filtered_queries_exact", "filtered_overflow_exact")


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def small(n=N, kind=H.VEC_QUANT8, seed=1):
    vs = rand_vectors(n, D, seed)
    return H.HNSW.new(8, 32, D, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(n, 8, seed))


def raw(index, s, Q, nq, n, ef, mask_of, lo, hi, ids="own", counts=None, dists=None):
    out_ids = np.full((max(nq, 1), max(n, 1)), 7, dtype=np.uint32) if isinstance(ids, str) else ids
    rc = _lib.lib().hnsw_search_batch_filtered_set_range(
        index._h, ptr(Q, f32p), nq, n, ef, None if s is None else s._s, ptr(mask_of, u32p), ptr(lo, u32p), ptr(hi, u32p),
        ptr(out_ids, u32p), ptr(dists, f32p), ptr(counts, u32p), None, None)
    return rc, out_ids


# ---- argument errors: decided before the device is touched, the outputs left as they were -----------------------------
def test_host_form_argument_errors_need_no_device():
    index, other = small(), small(seed=2)
    index.set_labels(np.arange(N, dtype=np.uint32) % 3)
    rng = np.random.default_rng(5)
    s = index.mask_set([rng.random(N) < 0.5, rng.random(N) < 0.2])
    foreign = other.mask_set([np.ones(N, dtype=bool)])
    Q = rand_vectors(6, D, 12)
    mo = np.array([0, 1, 0, MAX, 1, 0], dtype=np.uint32)
    lo = np.array([0, 1, 2, 0, 5, 0], dtype=np.uint32)
    hi = np.array([0, 1, 2, MAX, 4, 2], dtype=np.uint32)
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()

    def rc(**kw):
        a = dict(s=s, Q=Q, nq=6, n=5, ef=32, mo=mo, lo=lo, hi=hi)
        a.update(kw)
        counts, dists = np.full(6, 9, dtype=np.uint32), np.full((6, max(a["n"], 1)), 3.5, dtype=np.float32)
        code, ids = raw(index, a["s"], a["Q"], a["nq"], a["n"], a["ef"], a["mo"], a["lo"], a["hi"], ids=a.get("ids", "own"),
                        counts=counts, dists=dists)
        if code != _lib.OK:  # an error leaves every output as it was
            assert (counts == 9).all() and (dists == 3.5).all() and (ids is None or (ids == 7).all()), kw
        return code

    assert rc(Q=None) == _lib.ERR_ARG
    assert rc(ids=None) == _lib.ERR_ARG
    assert rc(s=None) == _lib.ERR_ARG
    assert b"mask set" in L.hnsw_last_error()
    assert rc(lo=None) == _lib.ERR_ARG
    assert b"label range" in L.hnsw_last_error()
    assert rc(hi=None) == _lib.ERR_ARG
    assert rc(s=foreign) == _lib.ERR_ARG
    assert b"another handle" in L.hnsw_last_error()
    for bad in (2, 3, MAX - 1):  # neither < n_masks nor HNSW_MASK_NONE
        m = mo.copy()
        m[4] = bad
        assert rc(mo=m) == _lib.ERR_ARG, bad
        assert b"query 4 names mask" in L.hnsw_last_error()
    assert rc(n=65) == _lib.ERR_ARG
    assert rc(n=300, ef=10) == _lib.ERR_ARG
    assert rc(nq=1 << 31, ids=np.full((6, 5), 7, dtype=np.uint32)) == _lib.ERR_ARG
    assert rc(nq=(1 << 31) - 1 + 2, mo=None, ids=np.full((6, 5), 7, dtype=np.uint32)) == _lib.ERR_ARG
    # nq == 0 is HNSW_OK whatever else is missing (but for the set); n == 0 zeroes the counts and launches nothing
    assert rc(nq=0) == _lib.OK and rc(nq=0, Q=None, ids=None, mo=None, lo=None, hi=None) == _lib.OK
    assert rc(nq=0, s=None) == _lib.ERR_ARG and rc(nq=0, s=foreign) == _lib.ERR_ARG
    counts = np.full(6, 9, dtype=np.uint32)
    code, ids = raw(index, s, Q, 6, 0, 32, mo, lo, hi, counts=counts)
    assert code == _lib.OK and (counts == 0).all() and (ids == 7).all()
    code, ids = raw(index, s, Q, 6, 0, 32, None, lo, hi, counts=None)  # mask_of NULL: row 0; counts are optional
    assert code == _lib.OK and (ids == 7).all()
    # ef' = 257 with a triple planned on the graph path (every one is, under -1): refused by the planner, on the host
    index.set_option("filter_exact_max", -1)
    assert rc(ef=257) == _lib.ERR_ARG and rc(n=1, ef=1000) == _lib.ERR_ARG
    assert b"graph path" in L.hnsw_last_error()
    index.set_option("filter_exact_max", 65536)
    after = {k: index.stat(k) for k in KEYS}
    # (the planner of the ef' = 257 calls counted the two rows on the host: no device, no upload, no call completed)
    assert after.pop("mask_set_recounts") <= 2 and before.pop("mask_set_recounts") == 0
    assert after == before
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    es = empty.mask_set(1, 10)
    assert raw(empty, es, Q, 6, 5, 32, None, lo, hi)[0] == _lib.ERR_EMPTY
    for x in (s, foreign, es):
        x.close()


def test_device_forms_argument_errors_need_no_device():
    index, other = small(), small(seed=2)
    s, foreign = index.mask_set([np.ones(N, dtype=bool)]), other.mask_set([np.ones(N, dtype=bool)])
    norows = index.mask_set(0)
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()
    fake = C.c_void_p(256)  # never dereferenced: every call below is refused first
    for fn, tail in ((L.hnsw_search_batch_filtered_set_range_device, ()),
                     (L.hnsw_search_batch_filtered_set_range_device_finish, (None,))):
        def call(h=index._h, dq=fake, nq=6, n=5, ef=32, st=s._s, mo=fake, lo=fake, hi=fake, ids=fake, stats=fake):
            return fn(h, dq, nq, n, ef, st, mo, lo, hi, ids, None, None, stats, None, *tail)
        assert call(dq=None) == _lib.ERR_ARG
        assert call(st=None) == _lib.ERR_ARG
        assert call(st=foreign._s) == _lib.ERR_ARG
        assert b"another handle" in L.hnsw_last_error()
        assert call(lo=None) == _lib.ERR_ARG
        assert b"label ranges" in L.hnsw_last_error()
        assert call(hi=None) == _lib.ERR_ARG
        assert call(ids=None) == _lib.ERR_ARG
        assert call(stats=None) == _lib.ERR_ARG
        assert call(nq=1 << 31) == _lib.ERR_ARG
        assert call(n=65, ef=65) == _lib.ERR_ARG
        assert call(ef=257) == _lib.ERR_ARG  # every query takes the graph path
        assert call(st=norows._s, mo=None) == _lib.ERR_ARG  # row 0 of a set without rows
        assert call(dq=None, nq=0, mo=None, lo=None, hi=None, ids=None, stats=None) == _lib.OK  # nq == 0
        assert call(nq=0, st=None) == _lib.ERR_ARG
        assert call(n=0, dq=None, lo=None, hi=None, ids=None, stats=None) == _lib.OK  # n == 0: nothing launched
        assert call(h=None) != _lib.OK
    assert {k: index.stat(k) for k in KEYS} == before
    for x in (s, foreign, norows):
        x.close()


# ---- the planner's decision is exact, on the host --------------------------------------------------------------------
def test_the_planner_counts_a_conjunction_exactly():
    """ef' = 257 is refused (HNSW_ERR_ARG, "graph path") iff the call's one triple is planned on the graph path, and that
    is decided before the device is touched: the refusal flips exactly between filter_exact_max = A - 1 and A, whichever
    side the planner walks (the range's slice of the sorted column, or the row's set bits), under deletions.  (At A the
    planner passes the call on: HNSW_OK with a GPU, a device error without one -- anything but HNSW_ERR_ARG.)"""
    index = small()
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 6, size=N).astype(np.uint32)
    index.set_labels(lab)
    rows = np.stack([rng.random(N) < 0.9, rng.random(N) < 0.05, rng.random(N) < 0.5])
    s = index.mask_set(rows)
    short = index.mask_set([rng.random(600) < 0.5])  # allow_bits below hnsw_len
    short_row = np.zeros(N, dtype=bool)
    short_row[:600] = np.unpackbits(short.read(0).view(np.uint8), bitorder="little")[:600].astype(bool)
    deleted = np.array([5, 17, 300, 599, 650])
    index.mark_deleted(deleted)
    alive = np.ones(N, dtype=bool)
    alive[deleted] = False
    Q = rand_vectors(1, D, 3)
    sides = set()
    for st, row_b, row in ((s, rows[0], 0), (s, rows[1], 1), (s, rows[2], 2), (short, short_row, 0)):
        for lo, hi in ((1, 1), (0, 4), (2, 5), (5, 5), (0, MAX - 1)):
            in_range = (lab >= lo) & (lab <= hi) & alive
            A = int((row_b & in_range).sum())
            sides.add("slice" if int(in_range.sum()) <= int((row_b & alive).sum()) else "row")
            for exact_max, refused in ((A - 1, True), (A, False)):
                index.set_option("filter_exact_max", exact_max)
                rc, _ = raw(index, st, Q, 1, 1, 257, np.array([row], dtype=np.uint32), np.array([lo], dtype=np.uint32),
                            np.array([hi], dtype=np.uint32))
                assert (rc == _lib.ERR_ARG) == refused, (row, lo, hi, A, exact_max, rc)
                if refused:
                    assert b"graph path" in _lib.lib().hnsw_last_error()
    assert sides == {"slice", "row"}
    s.close()
    short.close()


# ---- the Python wrapper --------------------------------------------------------------------------------------------
def test_python_wrapper_argument_handling():
    index = small()
    rng = np.random.default_rng(7)
    s = index.mask_set([rng.random(N) < 0.5, rng.random(N) < 0.2])
    Q = rand_vectors(6, D, 12)
    # n == 0 launches nothing: the wrapper's own handling is all that runs
    for mask_of in (None, [0, 1, -1, 0, H.MASK_NONE, 1], np.array([1] * 6)):  # None: row 0; -1 and MASK_NONE: no row
        got = index.search_batch_filtered_set_range(Q, 0, 32, s, mask_of, 1, 1)  # scalars broadcast
        assert got[0].shape == (6, 0) and got[1].shape == (6, 0) and (got[2] == 0).all() and got[4].shape == (6,)
    got = index.search_batch_filtered_set_range(Q, 0, 32, s, None, np.arange(6), np.full(6, MAX, dtype=np.uint64))
    assert (got[2] == 0).all()
    with pytest.raises(ValueError):
        index.search_batch_filtered_set_range(Q, 5, 32, s, [0, 1], 0, 1)  # one row per query
    with pytest.raises(ValueError):
        index.search_batch_filtered_set_range(Q, 5, 32, s, [0, 1, 0, 1, 0, -2], 0, 1)
    with pytest.raises(ValueError):
        index.search_batch_filtered_set_range(Q, 5, 32, s, None, [0, 1], 3)  # one range per query, or scalars
    with pytest.raises(ValueError):
        index.search_batch_filtered_set_range(Q, 5, 32, s, None, 0, -1)
    with pytest.raises(ValueError):
        index.search_batch_filtered_set_range(Q, 5, 32, s, None, 0, 2 ** 32)
    with pytest.raises(H.HnswError) as e:
        index.search_batch_filtered_set_range(Q[:, :5], 5, 32, s, None, 0, 1)
    assert e.value.code == _lib.ERR_BAD_DIM
    with pytest.raises(H.HnswError) as e:  # a row the set does not have: the library's error, before any device
        index.search_batch_filtered_set_range(Q, 5, 32, s, [0, 1, 2, 0, 1, 0], 0, 1)
    assert e.value.code == _lib.ERR_ARG
    for key in ("uploads", "filtered_set_range_calls", "label_words_uploaded", "mask_set_words_uploaded"):
        assert index.stat(key) == 0, key
    s.close()


# ---- ABI ----------------------------------------------------------------------------------------------------------
def c_type_of(decl):
    """a parameter of a prototype -> the ctypes type the binding must use.  Device pointers (d_*), the stream, the handle
    and the set are bound as void pointers: they are passed as integers or opaque handles, never as host arrays."""
    decl = re.sub(r"/\*.*?\*/", "", decl).strip()
    name = re.search(r"(\w+)$", decl).group(1)
    kind = decl[: -len(name)].replace("const", "").replace(" ", "")
    if name.startswith("d_") or kind in ("void*", "hnsw_index*", "hnsw_mask_set*"):
        assert kind.endswith("*"), decl
        return C.c_void_p
    return {"float*": f32p, "uint32_t*": u32p, "uint8_t*": u8p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32,
            "hnsw_query_stats*": C.POINTER(_lib.QueryStats)}[kind]


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
    assert len(_lib.SYMBOLS[NEW_SYMBOLS[0]][1]) == 14 and len(_lib.SYMBOLS[NEW_SYMBOLS[1]][1]) == 14
    assert len(_lib.SYMBOLS[NEW_SYMBOLS[2]][1]) == 15
    for method in ("search_batch_filtered_set_range", "search_batch_filtered_set_range_device",
                   "search_batch_filtered_set_range_device_finish"):
        assert hasattr(H.HNSW, method), method
    for key in ("filtered_set_range_calls", "filtered_set_range_groups"):
        assert small(n=50).stat(key) == 0


# ---- the kernels' resources ------------------------------------------------------------------------------------------
# Occupancy [waves/SIMD] of every instantiation of search_filtered.hip as compiled BEFORE the graph kernel read a mask
# row next to a label range (the same flags, -Rpass-analysis=kernel-resource-usage): the floor for every later compile.
# Keys: the template arguments as they are mangled -- <KIND, P, DS, R> of hx_filt_graph_kernel (KIND 1: f32, 0: 8-bit),
# <KIND> of hx_filt_scan_kernel.
OCCUPANCY_BEFORE = {
    "hx_filt_graph_kernelILi1ELi25ELi100ELi1E": 3, "hx_filt_graph_kernelILi1ELi25ELi100ELi2E": 3,
    "hx_filt_graph_kernelILi1ELi25ELi100ELi4E": 3,
    "hx_filt_graph_kernelILi1ELi32ELi128ELi1E": 3, "hx_filt_graph_kernelILi1ELi32ELi128ELi2E": 2,
    "hx_filt_graph_kernelILi1ELi32ELi128ELi4E": 2,
    "hx_filt_graph_kernelILi1ELi0ELi0ELi1E": 5, "hx_filt_graph_kernelILi1ELi0ELi0ELi2E": 4,
    "hx_filt_graph_kernelILi1ELi0ELi0ELi4E": 4,
    "hx_filt_graph_kernelILi0ELi4ELi100ELi1E": 4, "hx_filt_graph_kernelILi0ELi4ELi100ELi2E": 4,
    "hx_filt_graph_kernelILi0ELi4ELi100ELi4E": 4,
    "hx_filt_graph_kernelILi0ELi0ELi0ELi1E": 7, "hx_filt_graph_kernelILi0ELi0ELi0ELi2E": 7,
    "hx_filt_graph_kernelILi0ELi0ELi0ELi4E": 6,
    "hx_filt_compact_kernelE": 8, "hx_filt_scan_kernelILi0E": 7, "hx_filt_scan_kernelILi1E": 6, "hx_filt_merge_kernelE": 8,
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_filtered_kernels_keep_their_occupancy(tmp_path):
    src = os.path.join(ROOT, "hnsw_rs_amd", "csrc", "search_filtered.hip")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
           "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "filtered.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    occ, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"remark:\s+Occupancy \[waves/SIMD\]: (\d+)", line)
        if m and cur is not None and "hx_filt_" in cur:
            occ[cur] = int(m.group(1))
    assert len(occ) == len(OCCUPANCY_BEFORE) == 19, sorted(occ)  # no new kernel, no new instantiation
    for tag, floor in OCCUPANCY_BEFORE.items():
        names = [k for k in occ if tag in k]
        assert len(names) == 1, (tag, names)
        assert occ[names[0]] >= floor, (tag, occ[names[0]], floor)
