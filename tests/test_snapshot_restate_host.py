"""tests/snapshot_restate.py can fail (no GPU): its packing against bytes spelled out by hand from the layout comment of
hnsw_rs_amd/csrc/device_index.h, its restatement of a host-built index against Graph.csr(), and check_canonical
against an otherwise correct synthetic snapshot with one thing wrong at a time -- each must be rejected with a message
that names the array, row and slot."""
import numpy as np
import pytest

import hnsw_rs_amd as H
from oracle import oracle_py as O
from tests import snapshot_restate as R
from tests.util import rand_vectors

F = 0xFFFFFFFF
ONE, HALF = [0x00, 0x00, 0x80, 0x3F], [0x00, 0x00, 0x00, 0x3F]  # 1.0f, 0.5f little-endian


# ---- known answers ------------------------------------------------------------------------------------------------------

def test_quant8_row_d12_one_full_chunk_and_a_tail_of_four():
    """half = roundup16(8 + 4 + 4) = 16: half 0 [min][delta][codes 0..3][tail codes 8..11], half 1 [min][delta]
    [codes 4..7][4 zeros]"""
    codes = np.arange(100, 112, dtype=np.uint8)
    row = R.pack_q8_rows([1.0], [0.5], codes[None, :])[0]
    assert row.tolist() == ONE + HALF + [100, 101, 102, 103] + [108, 109, 110, 111] + \
        ONE + HALF + [104, 105, 106, 107] + [0, 0, 0, 0]
    assert R.half_bytes(12) == 16


def test_quant8_row_d7_no_full_chunk():
    """half = roundup16(8 + 0 + 7) = 16: half 0 [min][delta][tail codes 0..6][1 zero], half 1 [min][delta][8 zeros]"""
    codes = np.array([9, 8, 7, 6, 5, 4, 3], dtype=np.uint8)
    row = R.pack_q8_rows([0.5], [1.0], codes[None, :])[0]
    assert row.tolist() == HALF + ONE + [9, 8, 7, 6, 5, 4, 3] + [0] + HALF + ONE + [0] * 8


def test_quant8_row_d100_is_one_cache_line():
    """the comment's own example: half = 8 + 48 + 4 -> 64 B; chunk 11's codes 88..91 end half 0's chunks, the tail codes
    96..99 follow, the last four bytes (where an inline block keeps the neighbour's id) are zero"""
    codes = np.arange(100, dtype=np.uint8)
    row = R.pack_q8_rows([1.0], [0.5], codes[None, :])[0]
    assert len(row) == 128
    assert row[8:12].tolist() == [0, 1, 2, 3] and row[52:56].tolist() == [88, 89, 90, 91]
    assert row[56:64].tolist() == [96, 97, 98, 99, 0, 0, 0, 0]
    assert row[64 + 8:64 + 12].tolist() == [4, 5, 6, 7] and row[64 + 52:64 + 56].tolist() == [92, 93, 94, 95]
    assert row[64 + 56:].tolist() == [0] * 8


def test_f32_row_d5_is_padded_to_32_bytes():
    row = R.pack_f32_rows(np.array([[1.0, 0.5, 1.0, 1.0, 0.5]], dtype=np.float32))[0]
    assert row.tolist() == ONE + HALF + ONE + ONE + HALF + [0] * 12


def test_adjacency_row_with_exactly_S_ids_has_no_pointer():
    row, tail = R.pack_adj_row([70, 3, 12, 5, 9, 44, 1, 30], 8)
    assert row.tolist() == [1, 3, 5, 9, 12, 30, 44, 70] and tail is None
    row, tail = R.pack_adj_row([7, 2], 8)
    assert row.tolist() == [2, 7, F, F, F, F, F, F] and tail is None


def test_adjacency_row_with_S_plus_3_ids_keeps_S_minus_1_and_points_at_its_list():
    row, tail = R.pack_adj_row([70, 3, 12, 5, 9, 44, 1, 30, 81, 2, 99], 8, list_index=6)
    assert row.tolist() == [1, 2, 3, 5, 9, 12, 30, 0x80000006]
    assert tail.tolist() == [44, 70, 81, 99]


# ---- a host-built index restated -------------------------------------------------------------------------------------

def host_index(kind, d, m, n, extra):
    """n host-built points; `extra`: the first `extra` layer-0 rows get 20 more symmetric neighbours each (the recipe of
    test_insert_vec_with_overflowing_rows_and_inline_rows), so rows with and without overflow lists exist"""
    vs = rand_vectors(n, d, 31)
    lv = O.draw_levels(n, m, 5)
    index = H.HNSW.new(m, 8, d, kind).insert_bulk(vs, 1, False, levels=lv)
    if extra:
        ids, offs, nbrs = index.get_layer(0).csr()
        rows = [set(nbrs[int(offs[i]):int(offs[i + 1])].tolist()) for i in range(len(ids))]
        for i in range(extra):
            for k in range(20):
                j = (i + 7 * k + 1) % n
                rows[i].add(j)
                rows[j].add(i)
        flat = np.concatenate([np.array(sorted(r), dtype=np.uint32) for r in rows])
        o2 = np.zeros(len(ids) + 1, dtype=np.uint64)
        o2[1:] = np.cumsum([len(r) for r in rows])
        index.import_layer(0, ids, o2, flat)
    return index


@pytest.fixture(scope="module")
def q8():
    """(index, Host, its expected snapshot with inline rows): 8-bit, d = 20 (half = 32: 12 padding bytes), m = 4
    (S0 = 32, S1 = 8), 300 points, three or more layers"""
    index = host_index(H.VEC_QUANT8, 20, 4, 300, 100)
    host = R.Host(index)
    snap = R.expected_snapshot(index, inline=True, host=host)
    assert index.stat("uploads") == 0
    return index, host, snap


def copy_of(snap):
    return R.Snapshot([a.copy() for a in snap.arrays], snap.header.copy())


def pointer_row(snap, host):
    """the first layer-0 row that ends in an overflow pointer"""
    last = R.u32(snap.arrays[1]).reshape(host.n, host.S0)[:, -1]
    return int(np.nonzero((last != F) & (last >= 0x80000000))[0][0])


def short_row(snap, host):
    """the last layer-0 row with four ids or more and empty slots behind them"""
    k = (R.u32(snap.arrays[1]).reshape(host.n, host.S0) != F).sum(axis=1)
    return int(np.nonzero((k >= 4) & (k < host.S0))[0][-1])


def test_the_restatement_round_trips_to_the_host_graph(q8):
    index, host, snap = q8
    assert host.nb_layers >= 3 and (host.S0, host.S1, host.half, host.row_stride) == (32, 8, 32, 64)
    deg = np.diff(host.layers[0][1])
    assert (deg > 32).any() and (deg <= 32).any()  # rows with and without an overflow list
    assert [len(a) for a in snap.arrays] == host.sizes(int((deg > 32).sum()), int((deg[deg > 32] - 31).sum()), True)
    for l in range(host.nb_layers):
        got, want = R.decode_layer(snap, host, l), index.get_layer(l).csr()
        for g, w in zip(got, want):
            assert np.array_equal(g, w), "layer %d" % l
    R.check_canonical(snap, index, host)


def test_the_restatement_of_an_f32_index_without_overflow_lists():
    index = host_index(H.VEC_F32, 5, 16, 200, 0)
    host = R.Host(index)
    snap = R.expected_snapshot(index, host=host)
    assert (host.S0, host.S1, host.half, host.row_stride) == (32, 16, 0, 32)
    assert len(snap.arrays[4]) == 4 and R.u32(snap.arrays[5]).tolist() == [F] and len(snap.arrays[6]) == 0
    for l in range(host.nb_layers):
        for g, w in zip(R.decode_layer(snap, host, l), index.get_layer(l).csr()):
            assert np.array_equal(g, w), "layer %d" % l
    R.check_canonical(snap, index, host)
    v = np.zeros(5, dtype=np.float32)
    H._lib.check(index._L.hnsw_get_vector(index._h, 7, v.ctypes.data_as(H._lib.f32p)))
    assert snap.arrays[0][7 * 32:7 * 32 + 20].tobytes() == v.tobytes() and not snap.arrays[0][7 * 32 + 20:8 * 32].any()


def test_a_patched_snapshot_with_an_orphaned_list_is_canonical(q8):
    """what append_point leaves: a touched row points at a NEW list behind the old ones, its old list stays unused"""
    index, host, snap = q8
    s = copy_of(snap)
    adj0, off, lst = R.u32(s.arrays[1]).reshape(host.n, 32), R.u32(s.arrays[4]), R.u32(s.arrays[5])
    r = pointer_row(snap, host)
    li = int(adj0[r, -1] & 0x7FFFFFFF)
    tail = lst[off[li]:off[li + 1]]
    adj0[r, -1] = 0x80000000 | (len(off) - 1)
    s.arrays[4] = np.concatenate([off, [off[-1] + len(tail)]]).astype(np.uint32).view(np.uint8)
    s.arrays[5] = np.concatenate([lst, tail]).astype(np.uint32).view(np.uint8)
    fat = R.u32(s.arrays[6]).reshape(host.n, 32, 16)
    fat[r, 31, (32 - 4) // 4] = adj0[r, -1]
    R.check_canonical(s, index, host)


# ---- one thing wrong at a time ------------------------------------------------------------------------------------------

def reject(snap, index, host, pattern):
    with pytest.raises(R.SnapshotMismatch, match=pattern):
        R.check_canonical(snap, index, host)


def test_two_ids_swapped_in_a_row(q8):
    index, host, snap = q8
    s = copy_of(snap)
    adj0 = R.u32(s.arrays[1]).reshape(host.n, 32)
    adj0[17, [4, 5]] = adj0[17, [5, 4]]
    reject(s, index, host, r"adj0 row 17 slot 5: ids not ascending")


def test_a_hole_in_the_middle_of_a_row(q8):
    index, host, snap = q8
    s = copy_of(snap)
    adj_up = R.u32(s.arrays[2]).reshape(-1, 8)
    r = int(np.nonzero(adj_up[:, 1] != F)[0][0])  # an upper row with two ids or more
    adj_up[r, 0] = F
    reject(s, index, host, r"adj_up row %d \(node \d+, layer \d+\) slot 0: a hole" % r)
    s = copy_of(snap)
    r = short_row(snap, host)
    R.u32(s.arrays[1]).reshape(host.n, 32)[r, 2] = F
    reject(s, index, host, r"adj0 row %d slot 2: a hole" % r)


def test_a_dangling_overflow_index(q8):
    index, host, snap = q8
    s = copy_of(snap)
    adj0 = R.u32(s.arrays[1]).reshape(host.n, 32)
    n_lists = len(s.arrays[4]) // 4 - 1
    r = pointer_row(snap, host)
    adj0[r, 31] = 0x80000000 | n_lists
    reject(s, index, host, r"adj0 row %d slot 31: overflow list %d of %d lists" % (r, n_lists, n_lists))


def test_an_overflow_pointer_outside_the_last_slot(q8):
    index, host, snap = q8
    s = copy_of(snap)
    adj0 = R.u32(s.arrays[1]).reshape(host.n, 32)
    r = pointer_row(snap, host)
    adj0[r, 30], adj0[r, 31] = adj0[r, 31], F
    reject(s, index, host, r"adj0 row %d slot 30: an overflow pointer" % r)


def test_an_overflow_list_that_repeats_an_in_row_id(q8):
    index, host, snap = q8
    s = copy_of(snap)
    adj0, off, lst = R.u32(s.arrays[1]).reshape(host.n, 32), R.u32(s.arrays[4]), R.u32(s.arrays[5])
    r = pointer_row(snap, host)
    li = int(adj0[r, 31] & 0x7FFFFFFF)
    assert off[li + 1] - off[li] >= 2
    lst[off[li]] = adj0[r, 30]
    reject(s, index, host, r"adj0 row %d: overflow list %d starts at %d, not above the last in-row id %d" % (
        r, li, adj0[r, 30], adj0[r, 30]))
    s = copy_of(snap)  # ... and a list whose second id repeats its first
    lst = R.u32(s.arrays[5])
    lst[off[li] + 1] = lst[off[li]]
    reject(s, index, host, r"adj0 row %d: overflow list %d does not ascend" % (r, li))


def test_an_overflow_list_that_lost_an_id(q8):
    index, host, snap = q8
    s = copy_of(snap)
    adj0, off, lst = R.u32(s.arrays[1]).reshape(host.n, 32), R.u32(s.arrays[4]), R.u32(s.arrays[5])
    r = pointer_row(snap, host)
    li = int(adj0[r, 31] & 0x7FFFFFFF)
    lst[off[li + 1] - 1] += 1  # still ascending, no longer the host's neighbour
    reject(s, index, host, r"adj0 row %d: overflow list %d holds" % (r, li))


def test_a_row_that_is_not_the_hosts(q8):
    index, host, snap = q8
    s = copy_of(snap)
    adj0 = R.u32(s.arrays[1]).reshape(host.n, 32)
    r = short_row(snap, host)
    k = int((adj0[r] != F).sum())
    assert adj0[r, k - 1] < 299
    adj0[r, k] = 299  # ascending, one neighbour too many
    reject(s, index, host, r"adj0 row %d slot %d: holds" % (r, k))


def test_one_flipped_byte_in_the_padding_of_a_row(q8):
    index, host, snap = q8
    s = copy_of(snap)
    assert s.arrays[0][41 * 64 + 63] == 0
    s.arrays[0][41 * 64 + 63] ^= 0x10  # the last padding byte of half 1
    reject(s, index, host, r"rows row 41 byte 63: holds 0x10, expected 0x00")


def test_one_inline_slot_holding_a_stale_neighbour_row(q8):
    index, host, snap = q8
    s = copy_of(snap)
    fat = s.arrays[6].reshape(host.n, 32, 64)
    adj0 = R.u32(s.arrays[1]).reshape(host.n, 32)
    other = (int(adj0[9, 2]) + 1) % host.n
    fat[9, 2] = s.arrays[0].reshape(host.n, 64)[other]
    fat[9, 2, 28:32] = adj0[9, 2:3].view(np.uint8)  # the id word is right: only the copied row is another point's
    reject(s, index, host, r"inline rows node 9 slot 2 word \d+: holds")
    s = copy_of(snap)  # ... and an empty slot that is not all zero apart from its id word
    fat = s.arrays[6].reshape(host.n, 32, 64)
    r = short_row(snap, host)
    fat[r, 31, 0] = 1
    reject(s, index, host, r"inline rows node %d slot 31 word 0: holds 0x00000001, expected 0x00000000" % r)


def test_an_upper_base_range_overlapping_another(q8):
    index, host, snap = q8
    s = copy_of(snap)
    ub = R.u32(s.arrays[3])
    up = np.nonzero(host.levels > 0)[0]
    a, b = int(up[2]), int(up[3])
    ub[b] = ub[a]
    reject(s, index, host, r"upper_base\[%d\] = %d: its range \[\d+, \d+\) overlaps the range \[\d+, \d+\) of node %d" % (
        b, ub[a], a))
    s = copy_of(snap)
    ub = R.u32(s.arrays[3])
    lvl0 = int(np.nonzero(host.levels == 0)[0][5])
    ub[lvl0] = 0
    reject(s, index, host, r"upper_base\[%d\]: a level-0 node holds 0x00000000" % lvl0)
    s = copy_of(snap)  # off by one for a single node: its range runs into its successor's
    ub = R.u32(s.arrays[3])
    ub[a] += 1
    reject(s, index, host, r"upper_base\[\d+\]")


def test_a_live_size_one_row_short(q8):
    index, host, snap = q8
    for i, unit in ((0, 64), (1, 32 * 4), (2, 8 * 4), (3, 4), (6, 32 * 64)):
        s = copy_of(snap)
        s.arrays[i] = s.arrays[i][:-unit]
        reject(s, index, host, r"%s \(array %d\): live size %d, expected %d" % (
            R.NAMES[i], i, len(snap.arrays[i]) - unit, len(snap.arrays[i])))
    s = copy_of(snap)  # one id short in the lists
    s.arrays[5] = s.arrays[5][:-4]
    reject(s, index, host, r"ovf_nbrs \(array 5\): live size")


def test_a_wrong_header_word(q8):
    index, host, snap = q8
    s = copy_of(snap)
    s.header[6] = (int(s.header[6]) + 1) % host.n
    reject(s, index, host, r"header word 6 \(ep\)")
    s = copy_of(snap)
    s.header[4] -= 1
    reject(s, index, host, r"header word 4 \(n_points\)")
