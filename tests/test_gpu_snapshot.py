"""The live HBM snapshot, read back whole through hnsw_snapshot_describe and held to tests/snapshot_restate.py after
each of the three ways it is written: DeviceIndex::upload (a), DeviceIndex::append_point with hx_patch_kernel and
hx_fat_rebuild_kernel (b, d), and the on-device build, whose working adjacency stays in HBM and is sorted in place and
patched by refresh_rows (c).  Every row of every array is compared, bitwise: a wrong word in a row no query visits, a
tail grow() left unfilled, an inline block that disagrees with its adjacency row or a live size that is off by one
changes no search answer at these sizes, and all of them fail here."""
import numpy as np
import pytest

import hnsw_rs_amd as H
from oracle import oracle_py as O
from tests import snapshot_restate as R
from tests.kernel_matrix import N_POINTS
from tests.util import rand_vectors

pytestmark = pytest.mark.gpu

Q8, F32 = H.VEC_QUANT8, H.VEC_F32


def matrix_index(kind, d, m):
    """the fixture recipe of tests/kernel_matrix.py: N_POINTS host-built points (an index of its own: these tests insert)"""
    vs = H.synth_rows(0, 0x3A7F0000 + d * 256 + m, 0, N_POINTS, d)
    lv = O.draw_levels(N_POINTS, m, 0x3A7F + d)
    return H.HNSW.new(m, 32, d, kind).insert_bulk(vs, 8, False, levels=lv)


def overflow_index():
    """the recipe of test_insert_vec_with_overflowing_rows_and_inline_rows: d = 20, m = 4, n = 400, every layer-0 row
    with 20 more symmetric neighbours than the build gave it, through import_layer -- rows above the 32-slot stride"""
    d, m, n0 = 20, 4, 400
    vs = rand_vectors(n0, d, 21)
    lv = O.draw_levels(n0, m, 4)
    index = H.HNSW.new(m, 8, d, Q8).insert_bulk(vs, 1, False, levels=lv)
    ids, offs, nbrs = index.get_layer(0).csr()
    rows = [set(nbrs[int(offs[i]):int(offs[i + 1])].tolist()) for i in range(len(ids))]
    for i in range(n0):
        for k in range(20):
            j = (i + 7 * k + 1) % n0
            rows[i].add(j)
            rows[j].add(i)
    flat = np.concatenate([np.array(sorted(r), dtype=np.uint32) for r in rows])
    o2 = np.zeros(len(ids) + 1, dtype=np.uint64)
    o2[1:] = np.cumsum([len(r) for r in rows])
    index.import_layer(0, ids, o2, flat)
    return index


# (id, kind, d, m, the inline_rows option, array 6 exists).  Inline rows are an 8-bit, 32-slot layout that needs four
# spare bytes at the end of half 0: d = 7 (15 of 16 bytes used) and m = 24 (64-slot rows) have none, asked for or not.
CASES = [
    ("q8-d7", Q8, 7, 16, 1, False), ("q8-d36", Q8, 36, 16, 1, True), ("q8-d100", Q8, 100, 16, 1, True),
    ("q8-d128", Q8, 128, 16, 1, True), ("q8-d36-compact", Q8, 36, 16, 0, False),
    ("f32-d5", F32, 5, 16, 0, False), ("f32-d37", F32, 37, 16, 0, False), ("f32-d100", F32, 100, 16, 0, False),
    ("f32-d128", F32, 128, 16, 0, False),
    ("q8-d100-m24", Q8, 100, 24, 1, False), ("f32-d37-m24", F32, 37, 24, 0, False),
    ("overflow-inline", Q8, 20, 4, 1, True), ("overflow-compact", Q8, 20, 4, 0, False),
]
IDS = [c[0] for c in CASES]
_BASE = {}


def case_index(name, kind, d, m, inline):
    """a fresh clone of the case's host-built index (built once per process), its inline_rows option set"""
    key = (kind, d, m)
    if key not in _BASE:
        _BASE[key] = overflow_index() if name.startswith("overflow") else matrix_index(kind, d, m)
    index = _BASE[key].clone()
    index.set_option("inline_rows", inline)
    return index


def read(index):
    """the snapshot as it stands: hnsw_snapshot_describe uploads silently when the snapshot is stale, which would
    hand back a fresh upload instead of what the patches (or the build) left"""
    before = index.stat("uploads"), index.stat("patch_fallbacks")
    snap = R.read_snapshot(index)
    assert (index.stat("uploads"), index.stat("patch_fallbacks")) == before, "reading the snapshot uploaded it"
    return snap


def assert_is_the_restatement(snap, index, inline):
    """all seven arrays and the header, byte for byte; upper_base validated, then taken from the snapshot"""
    host = R.Host(index)
    assert (len(snap.arrays[6]) != 0) == inline, "inline rows: %d bytes" % len(snap.arrays[6])
    R.validate_upper_base(R.u32(snap.arrays[3]), host.levels, host.S1, len(snap.arrays[2]))
    want = R.expected_snapshot(index, upper_base=R.u32(snap.arrays[3]), inline=inline, host=host)
    R.assert_same_bytes(snap, want)
    R.check_canonical(snap, index, host)
    return host


# ---- a. a fresh upload --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kind,d,m,inline,fat", CASES, ids=IDS)
def test_a_fresh_upload_is_the_restatement_byte_for_byte(name, kind, d, m, inline, fat):
    index = case_index(name, kind, d, m, inline)
    index.upload()
    assert index.stat("uploads") == 1
    host = assert_is_the_restatement(read(index), index, fat)
    assert host.S0 == (64 if m == 24 else 32)
    if name.startswith("overflow"):
        assert (np.diff(host.layers[0][1]) > 32).all()  # every layer-0 row has an overflow list


# ---- b. a patched snapshot ----------------------------------------------------------------------------------------------

def same_but_for_pointers(got, want, host):
    """arrays 0 to 3 of a patched snapshot against a fresh upload's: equal, except that an adjacency slot that holds an
    overflow pointer holds one in both, to lists numbered differently"""
    R.assert_same_bytes(got, want, arrays=(0, 3), header=True)
    for i, S in ((1, host.S0), (2, host.S1)):
        a, b = R.u32(got.arrays[i]), R.u32(want.arrays[i])
        assert len(a) == len(b), "%s: %d words, a fresh upload has %d" % (R.NAMES[i], len(a), len(b))
        pa, pb = (a != R.EMPTY) & (a >= R.OVF), (b != R.EMPTY) & (b >= R.OVF)
        bad = np.nonzero((pa != pb) | (~pa & (a != b)))[0]
        assert bad.size == 0, "%s row %d slot %d: 0x%08X, a fresh upload holds 0x%08X" % (
            R.NAMES[i], bad[0] // S, bad[0] % S, a[bad[0]], b[bad[0]])


def insert_and_check(index, new, levels, fat, always=()):
    """insert_vec new[i] at levels[i], check_canonical after the first insertion, at every step where device_bytes()
    changed (an array moved there), at the steps of `always` and at the end -> the steps after which an array had moved"""
    up0 = index.stat("uploads")
    patches0 = index.stat("point_patches")
    n0, bytes_before, grown = index.len(), index.device_bytes(), []
    with H.kernel_log() as log:
        for i in range(len(new)):
            assert index.insert_vec(new[i], level=int(levels[i])) == n0 + i
            now = index.device_bytes()
            if now != bytes_before:
                grown.append(i)
                bytes_before = now
            if i == 0 or i in always or i == len(new) - 1 or grown[-1:] == [i]:
                try:
                    snap = read(index)
                    assert (len(snap.arrays[6]) != 0) == fat
                    R.check_canonical(snap, index)
                except AssertionError as e:
                    raise AssertionError("after insertion %d (arrays moved at %s): %s" % (i, grown, e)) from None
    assert index.stat("uploads") == up0, "an insert_vec threw the snapshot away"
    assert index.stat("point_patches") - patches0 == len(new) and index.stat("patch_fallbacks") == 0
    assert "hx_patch_kernel" in log, dict(log)
    assert ("hx_fat_rebuild_kernel" in log) == fat, dict(log)
    return grown


@pytest.mark.parametrize("name,kind,d,m,inline,fat", CASES, ids=IDS)
def test_a_patched_snapshot_stays_canonical(name, kind, d, m, inline, fat):
    """400 insert_vec calls with drawn levels on a live snapshot: the row and adjacency arrays have no room behind a
    fresh upload, so they grow (capacity + 1/8 + 4 KiB, copied device to device, the tail filled) at the first
    insertion and again later; one insertion opens two top layers and moves the entry point"""
    index = case_index(name, kind, d, m, inline)
    steps, top = 400, 230
    new = rand_vectors(steps, d, 22) if name.startswith("overflow") else H.synth_rows(0, 0x5EED0009, 0, steps, d)
    levels = O.draw_levels(steps, m, 11)
    index.upload()
    layers0 = index.nb_layers()
    levels[top] = layers0 + 1
    grown = insert_and_check(index, new, levels, fat, always=(top, top + 1))
    assert grown[0] == 0 and len(grown) >= 2, grown  # the arrays moved at the first insertion and again later
    assert index.nb_layers() == layers0 + 2 and int(index.params.ep) == index.len() - steps + top
    snap = read(index)
    host = R.check_canonical(snap, index)
    assert snap.header[5] == layers0 + 2 and snap.header[6] == int(index.params.ep)
    if name.startswith("overflow"):
        assert len(snap.arrays[4]) // 4 - 1 > 400  # lists were appended behind the 400 of the upload
    fresh = index.clone()
    fresh.upload()
    same_but_for_pointers(snap, read(fresh), host)


# ---- c. the snapshot a device build leaves behind --------------------------------------------------------------------------

def device_built(kind, d, m, n, seed, level_seed):
    vs = H.synth_rows(0, seed, 0, n, d)
    lv = O.draw_levels(n, m, level_seed)
    index = H.HNSW.new(m, 32, d, kind)
    with H.kernel_log() as log:
        index.insert_bulk_device(vs, 8, False, levels=lv)
    assert index.stat("build_cpu_path_points") == 0
    # the build appends and prunes rows in the order of its edge records: the snapshot it keeps was sorted row by row
    assert "hx_sort_rows_kernel" in log, dict(log)
    return index


# points of the m = 5 build: the seed is 2048 points and its clamp already leaves kept-last-edge records (4 at
# n = 2200 and 2500, 8 at 3000, 21 at 8000), so a few hundred device-inserted points are enough
KEPT_LAST_N = 2500


def f32_d33():
    """f32, d = 33, m = 16, n = 3000: the seed is 2048 points, the device inserts the rest"""
    return device_built(F32, 33, 16, 3000, 0xB17D0000 + 33 * 1000 + 16, 0xB17D + 16)


def assert_retained_is_the_restatement(index):
    up = index.stat("uploads")
    snap = R.read_snapshot(index)
    assert index.stat("uploads") == up, "the build's snapshot was not kept: describing it uploaded a fresh one"
    assert len(snap.arrays[4]) == 4  # no overflow lists: all seven arrays are comparable
    assert_is_the_restatement(snap, index, False)


def test_the_snapshot_a_device_build_leaves_is_the_restatement_byte_for_byte():
    assert_retained_is_the_restatement(f32_d33())


def test_the_snapshot_of_a_device_build_with_kept_last_edges_is_the_restatement():
    """the m = 5 recipe of test_small_m_clamps_the_seed_and_mirrors_kept_last_edges: edges kept because they were a
    row's last one are mirrored on the host after the read-back, and refresh_rows copies those rows over the build's"""
    index = device_built(Q8, 100, 5, KEPT_LAST_N, 0xB17D0005, 0xB17D05)
    assert index.stat("build_kept_last_edges") > 0
    assert_retained_is_the_restatement(index)


# ---- d. patching on top of a retained build snapshot ---------------------------------------------------------------------

def test_patching_a_retained_build_snapshot_stays_canonical():
    index = f32_d33()
    up = index.stat("uploads")
    new = H.synth_rows(0, 0x5EED0009, 0, 50, 33)
    grown = insert_and_check(index, new, O.draw_levels(50, 16, 11), False)
    assert grown[:1] == [0] and index.stat("uploads") == up
    fresh = index.clone()
    fresh.upload()
    same_but_for_pointers(read(index), read(fresh), R.Host(index))
