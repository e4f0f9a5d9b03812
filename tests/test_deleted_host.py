"""Deletion on the host (include/hnsw_mi355x.h, "deletion"): the set itself, what carries it (clone, save / load) and
what leaves it alone (inserts), the sidecar file `deleted` against an independent reader, and the resources of the
mask's scatter kernel.  None of these needs a GPU."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests.util import rand_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def small(n=700, d=12, kind=H.VEC_QUANT8, seed=1):
    vs = rand_vectors(n, d, seed)
    return H.HNSW.new(8, 32, d, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(n, 8, seed)), vs


def read_sidecar(path):
    """independent reader of <dir>/deleted: u64 count, then count u32 ids, big-endian"""
    b = open(path, "rb").read()
    (count,) = struct.unpack(">Q", b[:8])
    assert len(b) == 8 + 4 * count
    return list(struct.unpack(">%dI" % count, b[8:]))


def test_mark_unmark_is_count_get():
    index, _ = small()
    assert index.deleted_count() == 0 and index.deleted_ids().size == 0 and index.stat("deleted") == 0
    index.mark_deleted([5, 64, 63, 699, 5])
    index.mark_deleted(64)  # idempotent
    assert index.deleted_count() == 4 and index.stat("deleted") == 4
    assert index.deleted_ids().tolist() == [5, 63, 64, 699]
    assert index.is_deleted(63) and not index.is_deleted(62)
    index.unmark_deleted([63, 62, 63])  # unmarking a live id is a no-op too
    assert index.deleted_ids().tolist() == [5, 64, 699]
    index.unmark_deleted(index.deleted_ids())
    assert index.deleted_count() == 0 and not index.is_deleted(5)


def test_out_of_range_leaves_the_set_unchanged():
    index, _ = small()
    index.mark_deleted([1, 2, 3])
    for call in (index.mark_deleted, index.unmark_deleted):
        with pytest.raises(H.HnswError) as e:
            call([4, 2, 700, 9])
        assert e.value.code == _lib.ERR_ARG
        assert index.deleted_ids().tolist() == [1, 2, 3]
    with pytest.raises(H.HnswError) as e:
        index.is_deleted(700)
    assert e.value.code == _lib.ERR_ARG


def test_get_deleted_respects_cap():
    import ctypes as C
    index, _ = small()
    index.mark_deleted([9, 3, 600])
    out = np.full(4, 7, dtype=np.uint32)
    n = C.c_uint64()
    assert index._L.hnsw_get_deleted(index._h, out.ctypes.data_as(_lib.u32p), 2, C.byref(n)) == 0
    assert n.value == 3 and out.tolist() == [3, 9, 7, 7]


def test_clone_carries_the_set_and_is_independent():
    index, _ = small()
    index.mark_deleted([10, 20, 30])
    c = index.clone()
    assert c.deleted_ids().tolist() == [10, 20, 30]
    c.mark_deleted([40])
    index.unmark_deleted([10])
    assert c.deleted_ids().tolist() == [10, 20, 30, 40] and index.deleted_ids().tolist() == [20, 30]


def test_inserts_leave_the_set_alone():
    index, vs = small(n=640)  # 640 = 10 words exactly: the new ids start a new word
    index.mark_deleted([0, 639, 100])
    new_id = index.insert_vec(rand_vectors(1, vs.shape[1], 5)[0])
    assert new_id == 640 and not index.is_deleted(640)
    index.insert_bulk(rand_vectors(100, vs.shape[1], 6), 2, False)
    assert index.len() == 741
    assert index.deleted_ids().tolist() == [0, 100, 639]
    assert not any(index.is_deleted(i) for i in range(640, 741))
    index.mark_deleted([740])  # the new ids can be deleted in turn
    assert index.deleted_ids().tolist() == [0, 100, 639, 740]


@pytest.mark.parametrize("kind", [H.VEC_QUANT8, H.VEC_F32])
def test_save_load_with_deletions(tmp_path, kind):
    index, _ = small(kind=kind)
    plain, dele = str(tmp_path / "plain"), str(tmp_path / "dele")
    index.save(plain)
    ids = [0, 1, 77, 128, 699]
    index.mark_deleted(ids[::-1])
    index.save(dele)
    # the reference's files are byte-identical to those of the same index with nothing deleted
    for name in ["points", "params"] + ["layers/" + f for f in os.listdir(os.path.join(plain, "layers"))]:
        assert open(os.path.join(plain, name), "rb").read() == open(os.path.join(dele, name), "rb").read(), name
    assert sorted(os.listdir(dele)) == ["deleted", "layers", "params", "points"]
    assert sorted(os.listdir(plain)) == ["layers", "params", "points"]
    assert read_sidecar(os.path.join(dele, "deleted")) == ids
    back = H.HNSW.load(dele)
    assert back.deleted_ids().tolist() == ids and back.stat("deleted") == len(ids)
    assert H.HNSW.load(plain).deleted_count() == 0


def test_empty_set_writes_no_sidecar_and_removes_a_stale_one(tmp_path):
    index, _ = small()
    d = str(tmp_path / "x")
    index.mark_deleted([3])
    index.save(d)
    assert read_sidecar(os.path.join(d, "deleted")) == [3]
    index.unmark_deleted([3])
    shutil.rmtree(os.path.join(d, "layers"))  # (save refuses an existing layers/, as the reference does)
    index.save(d)
    assert sorted(os.listdir(d)) == ["layers", "params", "points"]
    assert H.HNSW.load(d).deleted_count() == 0


@pytest.mark.parametrize("damage", ["truncated", "trailing", "unsorted", "duplicate", "out_of_range", "short_header"])
def test_damaged_sidecar_is_refused(tmp_path, damage):
    index, _ = small()
    d = str(tmp_path / "x")
    index.save(d)
    good = [2, 40, 300]
    body = {
        "truncated": struct.pack(">Q3I", 4, *good),
        "trailing": struct.pack(">Q3I", 3, *good) + b"\0",
        "unsorted": struct.pack(">Q3I", 3, 40, 2, 300),
        "duplicate": struct.pack(">Q3I", 3, 2, 40, 40),
        "out_of_range": struct.pack(">Q3I", 3, 2, 40, 700),
        "short_header": b"\0\0\0",
    }[damage]
    with open(os.path.join(d, "deleted"), "wb") as f:
        f.write(body)
    with pytest.raises(H.HnswError) as e:
        H.HNSW.load(d)
    assert e.value.code == _lib.ERR_IO
    with open(os.path.join(d, "deleted"), "wb") as f:
        f.write(struct.pack(">Q3I", 3, *good))
    assert H.HNSW.load(d).deleted_ids().tolist() == good


def test_deletion_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()
    for name in ("hnsw_mark_deleted", "hnsw_unmark_deleted", "hnsw_is_deleted", "hnsw_deleted_count",
                 "hnsw_get_deleted"):
        assert re.search(r"\b%s\(" % name, header) and name in _lib.SYMBOLS, name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_mask_scatter_kernel_has_no_scratch_or_spills(tmp_path):
    src = os.path.join(ROOT, "hnsw_rs_amd", "csrc", "deleted_mask.hip")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
           "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "deleted_mask.o"),
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
    scatter = {k: v for k, v in kernels.items() if "hx_deleted_scatter_kernel" in k}
    assert len(scatter) == 1, sorted(kernels)
    for name, r in scatter.items():
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (name, r)
