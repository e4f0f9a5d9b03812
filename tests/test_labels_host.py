"""The label column on the host (include/hnsw_mi355x.h, "labels"): set / get against a numpy array, the errors that leave
it unchanged, what carries it (clone, save / load) and what leaves it alone (inserts), the sidecar file `labels` against
an independent reader, everything the three range-search entry points decide before they touch a device, and the C
prototypes against the ctypes binding.  None of this needs a GPU -- managing labels never does."""
import ctypes as C
import os
import re
import shutil
import struct

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests.util import rand_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 700, 12
f32p, u32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
NEW_SYMBOLS = ("hnsw_set_labels", "hnsw_get_labels", "hnsw_search_batch_filtered_range",
               "hnsw_search_batch_filtered_range_device", "hnsw_search_batch_filtered_range_device_finish")


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def small(n=N, kind=H.VEC_QUANT8, seed=1):
    vs = rand_vectors(n, D, seed)
    return H.HNSW.new(8, 32, D, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(n, 8, seed))


def read_sidecar(path):
    """independent reader of <dir>/labels: u64 count, then the u32 labels of ids 0..count-1, big-endian"""
    b = open(path, "rb").read()
    (count,) = struct.unpack(">Q", b[:8])
    assert len(b) == 8 + 4 * count
    return list(struct.unpack(">%dI" % count, b[8:]))


# ---- round trips ----------------------------------------------------------------------------------------------------
def test_set_and_get_round_trip_against_numpy():
    index = small()
    assert index.get_labels().tolist() == [0] * N  # never set: label 0
    rng = np.random.default_rng(3)
    ref = np.zeros(N, dtype=np.uint32)
    first = rng.integers(0, 2 ** 32, size=300, dtype=np.uint64).astype(np.uint32)
    index.set_labels(first)  # ids None: ids 0..k-1
    ref[:300] = first
    assert np.array_equal(index.get_labels(), ref)
    ids = rng.choice(N, 120, replace=False)
    vals = rng.integers(0, 1000, size=120).astype(np.uint32)
    index.set_labels(vals, ids)
    ref[ids] = vals
    assert np.array_equal(index.get_labels(), ref)
    assert np.array_equal(index.get_labels(ids), vals)
    assert np.array_equal(index.get_labels([699, 0, 699]), ref[[699, 0, 699]])
    index.set_labels([7, 8, 9], [5, 5, 5])  # the last one wins
    assert index.get_labels([5]).tolist() == [9]
    index.set_labels([0xFFFFFFFF], [N - 1])
    assert index.get_labels([N - 1]).tolist() == [0xFFFFFFFF]
    index.set_labels([], [])  # nothing to do
    assert index.get_labels(np.zeros(0, dtype=np.uint32)).shape == (0,)


def test_ids_added_later_have_label_zero():
    index = small(n=641)  # an odd length: the column's last 64-bit word is half used
    index.set_labels(np.arange(1, 642, dtype=np.uint32))
    new_id = index.insert_vec(rand_vectors(1, D, 5)[0])
    assert new_id == 641 and index.get_labels([641]).tolist() == [0]
    index.insert_bulk(rand_vectors(50, D, 6), 2, False)
    got = index.get_labels()
    assert got.shape == (692,) and np.array_equal(got[:641], np.arange(1, 642)) and not got[641:].any()
    index.set_labels([77], [691])  # the new ids take labels in turn
    assert index.get_labels([690, 691]).tolist() == [0, 77]


def test_out_of_range_leaves_every_label_unchanged():
    index = small()
    index.set_labels(np.arange(N, dtype=np.uint32) % 5)
    before = index.get_labels().copy()
    for ids in ([4, 2, N, 9], [N], [3, 0xFFFFFFFF]):
        with pytest.raises(H.HnswError) as e:
            index.set_labels(np.full(len(ids), 99, dtype=np.uint32), ids)
        assert e.value.code == _lib.ERR_ARG
        assert np.array_equal(index.get_labels(), before)
        with pytest.raises(H.HnswError) as e:
            index.get_labels(ids)
        assert e.value.code == _lib.ERR_ARG
    with pytest.raises(H.HnswError) as e:  # ids NULL names 0..k-1: k > len is an id >= len
        index.set_labels(np.full(N + 1, 99, dtype=np.uint32))
    assert e.value.code == _lib.ERR_ARG
    assert np.array_equal(index.get_labels(), before)
    L = _lib.lib()
    out = np.zeros(N + 1, dtype=np.uint32)
    assert L.hnsw_get_labels(index._h, None, N + 1, ptr(out, u32p)) == _lib.ERR_ARG
    assert L.hnsw_set_labels(None, None, ptr(out, u32p), 1) == _lib.ERR_ARG
    assert L.hnsw_set_labels(index._h, None, None, 1) == _lib.ERR_ARG
    assert L.hnsw_get_labels(index._h, None, 1, None) == _lib.ERR_ARG
    assert np.array_equal(index.get_labels(), before)
    for key in ("uploads", "label_words_uploaded", "filtered_range_calls", "filtered_range_ranges"):
        assert index.stat(key) == 0, key


def test_clone_carries_the_column_and_is_independent():
    index = small()
    lab = (np.arange(N, dtype=np.uint32) * 7) % 11
    index.set_labels(lab)
    c = index.clone()
    assert np.array_equal(c.get_labels(), lab)
    c.set_labels([500], [3])
    index.set_labels([600], [4])
    assert c.get_labels([3, 4]).tolist() == [500, lab[4]] and index.get_labels([3, 4]).tolist() == [lab[3], 600]


# ---- save / load --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [H.VEC_QUANT8, H.VEC_F32])
def test_save_load_round_trip(tmp_path, kind):
    index = small(kind=kind)
    plain, labelled = str(tmp_path / "plain"), str(tmp_path / "labelled")
    index.save(plain)
    lab = np.zeros(N, dtype=np.uint32)
    lab[[0, 1, 77, 128, 640]] = [5, 0xFFFFFFFF, 1, 2, 3]  # (trailing zero labels: the file may stop at id 640)
    index.set_labels(lab)
    index.save(labelled)
    # the other files are byte-identical to those of the same index without labels
    for name in ["points", "params"] + ["layers/" + f for f in os.listdir(os.path.join(plain, "layers"))]:
        assert open(os.path.join(plain, name), "rb").read() == open(os.path.join(labelled, name), "rb").read(), name
    assert sorted(os.listdir(labelled)) == ["labels", "layers", "params", "points"]
    assert sorted(os.listdir(plain)) == ["layers", "params", "points"]
    stored = read_sidecar(os.path.join(labelled, "labels"))
    assert 641 <= len(stored) <= N and stored == lab[: len(stored)].tolist()
    back = H.HNSW.load(labelled)
    assert np.array_equal(back.get_labels(), lab)
    assert not H.HNSW.load(plain).get_labels().any()
    # a full-length file is read as well
    with open(os.path.join(labelled, "labels"), "wb") as f:
        f.write(struct.pack(">Q%dI" % N, N, *lab.tolist()))
    assert np.array_equal(H.HNSW.load(labelled).get_labels(), lab)


def test_all_zero_labels_write_no_sidecar_and_remove_a_stale_one(tmp_path):
    index = small()
    d = str(tmp_path / "x")
    index.set_labels([9], [3])
    index.save(d)
    assert read_sidecar(os.path.join(d, "labels")) == [0, 0, 0, 9]
    index.set_labels([0], [3])  # every label zero again
    shutil.rmtree(os.path.join(d, "layers"))  # (save refuses an existing layers/, as the reference does)
    index.save(d)
    assert sorted(os.listdir(d)) == ["layers", "params", "points"]  # today's listing, the stale `labels` removed
    assert not H.HNSW.load(d).get_labels().any()


@pytest.mark.parametrize("damage", ["short_header", "truncated", "trailing", "count_above_len"])
def test_damaged_sidecar_is_refused(tmp_path, damage):
    index = small()
    d = str(tmp_path / "x")
    index.save(d)
    good = [2, 0, 300]
    body = {
        "short_header": b"\0\0\0",
        "truncated": struct.pack(">Q3I", 4, *good),
        "trailing": struct.pack(">Q3I", 3, *good) + b"\0",
        "count_above_len": struct.pack(">Q%dI" % (N + 1), N + 1, *([1] * (N + 1))),
    }[damage]
    with open(os.path.join(d, "labels"), "wb") as f:
        f.write(body)
    with pytest.raises(H.HnswError) as e:
        H.HNSW.load(d)
    assert e.value.code == _lib.ERR_IO
    with open(os.path.join(d, "labels"), "wb") as f:
        f.write(struct.pack(">Q3I", 3, *good))
    assert H.HNSW.load(d).get_labels()[:4].tolist() == good + [0]


# ---- the range searches: decided before the device is touched ---------------------------------------------------------
def raw_range(index, Q, nq, n, ef, lo, hi, ids="own", counts=None):
    out_ids = np.full((max(nq, 1), max(n, 1)), 7, dtype=np.uint32) if isinstance(ids, str) else ids
    rc = _lib.lib().hnsw_search_batch_filtered_range(index._h, ptr(Q, f32p), nq, n, ef, ptr(lo, u32p), ptr(hi, u32p),
                                                     ptr(out_ids, u32p), None, ptr(counts, u32p), None, None)
    return rc, out_ids


def test_range_search_argument_errors_need_no_device():
    index = small()
    index.set_labels(np.arange(N, dtype=np.uint32) % 3)
    Q = rand_vectors(6, D, 12)
    lo = np.array([0, 1, 2, 0, 5, 0], dtype=np.uint32)
    hi = np.array([0, 1, 2, 0xFFFFFFFF, 4, 2], dtype=np.uint32)
    keys = ("uploads", "label_words_uploaded", "filtered_range_calls", "filtered_range_ranges", "filtered_queries_graph",
            "filtered_queries_exact")
    before = {k: index.stat(k) for k in keys}

    def rc(**kw):
        a = dict(Q=Q, nq=6, n=5, ef=32, lo=lo, hi=hi)
        a.update(kw)
        return raw_range(index, a["Q"], a["nq"], a["n"], a["ef"], a["lo"], a["hi"], ids=a.get("ids", "own"))[0]

    assert rc(Q=None) == _lib.ERR_ARG
    assert rc(ids=None) == _lib.ERR_ARG
    assert rc(lo=None) == _lib.ERR_ARG
    assert b"label range" in _lib.lib().hnsw_last_error()
    assert rc(hi=None) == _lib.ERR_ARG
    assert rc(n=65) == _lib.ERR_ARG
    assert rc(n=300, ef=10) == _lib.ERR_ARG
    assert rc(nq=1 << 31, ids=np.zeros((6, 5), dtype=np.uint32)) == _lib.ERR_ARG
    # nq == 0 is HNSW_OK whatever else is missing; n == 0 zeroes the counts and launches nothing
    assert rc(nq=0) == _lib.OK and rc(nq=0, Q=None, ids=None, lo=None, hi=None) == _lib.OK
    counts = np.full(6, 9, dtype=np.uint32)
    code, ids = raw_range(index, Q, 6, 0, 32, lo, hi, counts=counts)
    assert code == _lib.OK and (counts == 0).all() and (ids == 7).all()
    got = index.search_batch_filtered_range(Q, 0, 32, 1, 1)  # scalars broadcast
    assert got[0].shape == (6, 0) and (got[2] == 0).all()
    # ef' = 257 with a range planned on the graph path (every range is, under -1): refused by the planner, on the host
    index.set_option("filter_exact_max", -1)
    assert rc(ef=257) == _lib.ERR_ARG and rc(n=1, ef=1000) == _lib.ERR_ARG
    assert b"graph path" in _lib.lib().hnsw_last_error()
    index.set_option("filter_exact_max", 65536)
    # the device form: its own limits and required buffers, before any device pointer is looked at
    L = _lib.lib()
    fake = C.c_void_p(256)  # never dereferenced: every call below is refused first
    for fn, tail in ((L.hnsw_search_batch_filtered_range_device, ()),
                     (L.hnsw_search_batch_filtered_range_device_finish, (None,))):
        assert fn(index._h, None, 6, 5, 32, fake, fake, fake, None, None, fake, None, *tail) == _lib.ERR_ARG
        assert fn(index._h, fake, 6, 5, 32, None, fake, fake, None, None, fake, None, *tail) == _lib.ERR_ARG  # d_lo
        assert fn(index._h, fake, 6, 5, 32, fake, None, fake, None, None, fake, None, *tail) == _lib.ERR_ARG  # d_hi
        assert fn(index._h, fake, 6, 5, 32, fake, fake, None, None, None, fake, None, *tail) == _lib.ERR_ARG  # d_ids
        assert fn(index._h, fake, 6, 5, 32, fake, fake, fake, None, None, None, None, *tail) == _lib.ERR_ARG  # d_stats
        assert fn(index._h, fake, 1 << 31, 5, 32, fake, fake, fake, None, None, fake, None, *tail) == _lib.ERR_ARG
        assert fn(index._h, fake, 6, 65, 65, fake, fake, fake, None, None, fake, None, *tail) == _lib.ERR_ARG
        assert fn(index._h, fake, 6, 5, 257, fake, fake, fake, None, None, fake, None, *tail) == _lib.ERR_ARG
        assert fn(index._h, None, 0, 5, 32, None, None, None, None, None, None, None, *tail) == _lib.OK  # nq == 0
        assert fn(None, fake, 6, 5, 32, fake, fake, fake, None, None, fake, None, *tail) != _lib.OK
    assert {k: index.stat(k) for k in keys} == before
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert raw_range(empty, Q, 6, 5, 32, lo, hi)[0] == _lib.ERR_EMPTY


def test_python_mirror_checks_the_ranges():
    index = small()
    Q = rand_vectors(6, D, 12)
    with pytest.raises(ValueError):
        index.search_batch_filtered_range(Q, 5, 32, [0, 1], 3)  # one entry per query, or a scalar
    with pytest.raises(ValueError):
        index.search_batch_filtered_range(Q, 5, 32, 0, -1)
    with pytest.raises(ValueError):
        index.search_batch_filtered_range(Q, 5, 32, 0, 2 ** 32)
    with pytest.raises(H.HnswError) as e:
        index.search_batch_filtered_range(Q[:, :5], 5, 32, 0, 1)
    assert e.value.code == _lib.ERR_BAD_DIM


# ---- ABI ----------------------------------------------------------------------------------------------------------
def c_type_of(decl):
    """a parameter of a prototype -> the ctypes type the binding must use.  Device pointers (d_*) and the stream are
    bound as void pointers: they are passed as integers, never as host arrays."""
    decl = re.sub(r"/\*.*?\*/", "", decl).strip()
    name = re.search(r"(\w+)$", decl).group(1)
    kind = decl[: -len(name)].replace("const", "").replace(" ", "")
    if name.startswith("d_") or kind == "void*" or kind == "hnsw_index*":
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
    for method in ("set_labels", "get_labels", "search_batch_filtered_range", "search_batch_filtered_range_device",
                   "search_batch_filtered_range_device_finish"):
        assert hasattr(H.HNSW, method), method
