"""The HBM snapshot restated in numpy from the layout comment of hnsw_rs_amd/csrc/device_index.h (and the header words
of hnsw_snapshot_desc, snapshot.cpp), and the checks that hold a live snapshot to it.  Nothing here calls product code
beyond the C ABI's accessors: hnsw_snapshot_describe to read a snapshot back, hnsw_get_params / hnsw_get_level /
hnsw_get_quant / hnsw_get_vector / hnsw_export_layer (Graph.csr) to restate one.

    read_snapshot(index)       the seven arrays over exactly their live sizes + the 32 header words, from HBM
    expected_snapshot(index)   the same, rebuilt from the host accessors: what a fresh upload must hold byte for byte
    check_canonical(snap, idx) the decoded comparison for a patched snapshot, whose overflow lists legitimately differ
                               from a fresh upload's (a patched row gets a NEW list, its old one is orphaned)

The layout, as this file states it (every word little-endian):
  0 rows        N x row_stride bytes.  8-bit: two halves of half_bytes = roundup16(8 + 4 (d / 8) + d % 8); half h holds
                [min f32][delta f32][codes 8c + 4h .. 8c + 4h + 3 of every full chunk c][h == 0: the d % 8 tail codes]
                [zeros].  f32: d floats, zeros up to roundup16(4 d).
  1 adj0        N x S0 u32, S0 = the power of two >= max(2 m, 32): ids ascending, then 0xFFFFFFFF.  More than S0 ids:
                the S0 - 1 smallest, then 0x80000000 | list.
  2 adj_up      max(1, sum of levels) x S1 u32, S1 = the power of two >= max(m, 8); row(id, l) = upper_base[id] + l - 1.
  3 upper_base  N u32, 0xFFFFFFFF for a level-0 node.
  4 ovf_off     lists + 1 u32, ovf_off[0] = 0: list i is ovf_nbrs[ovf_off[i] : ovf_off[i + 1]], the row's remaining ids
                ascending.  A fresh upload files the lists of layer 0 by id, then those of the upper rows by row index.
  5 ovf_nbrs    max(1, ids in lists) u32 (one 0xFFFFFFFF when there is no list).
  6 inline rows (optional) N x S0 x row_stride bytes: slot k of node i = the vector row of the id in adj0[i][k] with
                the raw adj0 word at byte half_bytes - 4; all zero apart from that word for an empty slot or a pointer.
upper_base is not exposed by the C ABI: it is validated structurally (validate_upper_base) and then taken from the
snapshot under test, or -- without a snapshot -- handed out in id order (upper_base_by_id)."""
import ctypes as C
from collections import namedtuple

import numpy as np

from hnsw_rs_amd import _lib

EMPTY = 0xFFFFFFFF
OVF = 0x80000000
MAGIC = 0x48584E53
NAMES = ("rows", "adj0", "adj_up", "upper_base", "ovf_off", "ovf_nbrs", "inline rows")
# the words of hnsw_snapshot_desc.header that are in use (the other 14 are zero)
HEADER_WORDS = ("magic", "version", "kind", "dim", "n_points", "nb_layers", "ep", "S0", "S1", "row_stride", "half_bytes",
                "nch4", "rem", "fat_stride_lo", "fat_stride_hi", "m", "ef_cons", "flags")

# arrays: seven flat uint8 arrays of exactly the live sizes (an absent array has length 0); header: uint32 [32]
Snapshot = namedtuple("Snapshot", "arrays header")


class SnapshotMismatch(AssertionError):
    """a snapshot that is not the canonical form of its host graph; the message names the array, row and slot"""


def _fail(fmt, *args):
    raise SnapshotMismatch(fmt % args)


def _up16(x):
    return (x + 15) & ~15


def _pow2_at_least(x, lowest):
    s = lowest
    while s < x:
        s *= 2
    return s


def half_bytes(d):
    return _up16(8 + 4 * (d // 8) + d % 8)


def u32(a):
    return np.ascontiguousarray(a).view("<u4")


# ---- single rows, as the layout comment spells them (the known-answer tests of test_snapshot_restate_host.py) ----------

def pack_q8_rows(mins, deltas, codes):
    """codes uint8 [n, d] -> uint8 [n, 2 half_bytes(d)]"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n, d = codes.shape
    nch, rem, half = d // 8, d % 8, half_bytes(d)
    out = np.zeros((n, 2, half), dtype=np.uint8)
    head = np.stack([np.asarray(mins, dtype="<f4"), np.asarray(deltas, dtype="<f4")], axis=1).view(np.uint8).reshape(n, 8)
    chunks = codes[:, :8 * nch].reshape(n, nch, 8)
    for h in (0, 1):
        out[:, h, :8] = head
        out[:, h, 8:8 + 4 * nch] = chunks[:, :, 4 * h:4 * h + 4].reshape(n, 4 * nch)
    out[:, 0, 8 + 4 * nch:8 + 4 * nch + rem] = codes[:, 8 * nch:]
    return out.reshape(n, 2 * half)


def pack_f32_rows(vals):
    """float32 [n, d] -> uint8 [n, roundup16(4 d)]"""
    vals = np.ascontiguousarray(vals, dtype="<f4")
    n, d = vals.shape
    out = np.zeros((n, _up16(4 * d)), dtype=np.uint8)
    out[:, :4 * d] = vals.view(np.uint8).reshape(n, 4 * d)
    return out


def pack_adj_row(ids, S, list_index=None):
    """one adjacency row -> (uint32 [S], the ids that go to its overflow list or None); list_index: the list's number,
    needed when there are more than S ids"""
    ids = np.sort(np.asarray(ids, dtype=np.uint32))
    out = np.full(S, EMPTY, dtype=np.uint32)
    if len(ids) <= S:
        out[:len(ids)] = ids
        return out, None
    out[:S - 1] = ids[:S - 1]
    out[S - 1] = OVF | list_index
    return out, ids[S - 1:]


# ---- the host side ----------------------------------------------------------------------------------------------------

class Host:
    """what the host accessors say about an index, read once: parameters, levels, packed vector rows, every layer's CSR"""

    def __init__(self, index):
        L, h = index._L, index._h
        p = index.params
        self.kind, self.d, self.m, self.ef_cons = int(p.vec_kind), int(p.dim), int(p.m), int(p.ef_cons)
        self.ep = int(p.ep)
        self.n = n = index.len()
        self.nb_layers = index.nb_layers()
        self.q8 = self.kind == _lib.VEC_QUANT8
        self.S0 = _pow2_at_least(int(p.mmax0), 32)
        self.S1 = _pow2_at_least(self.m, 8)
        self.half = half_bytes(self.d) if self.q8 else 0
        self.row_stride = 2 * self.half if self.q8 else _up16(4 * self.d)
        d = self.d
        self.levels = np.zeros(n, dtype=np.uint32)
        for i in range(n):
            _lib.check(L.hnsw_get_level(h, i, C.cast(self.levels.ctypes.data + 4 * i, _lib.u32p)))
        if self.q8:
            codes = np.zeros((n, d), dtype=np.uint8)
            mins, deltas = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
            for i in range(n):
                _lib.check(L.hnsw_get_quant(h, i, C.cast(codes.ctypes.data + i * d, _lib.u8p),
                                            C.cast(mins.ctypes.data + 4 * i, _lib.f32p),
                                            C.cast(deltas.ctypes.data + 4 * i, _lib.f32p)))
            self.rows = pack_q8_rows(mins, deltas, codes)
        else:
            vals = np.zeros((n, d), dtype=np.float32)
            for i in range(n):
                _lib.check(L.hnsw_get_vector(h, i, C.cast(vals.ctypes.data + 4 * i * d, _lib.f32p)))
            self.rows = pack_f32_rows(vals)
        # per layer: (node ids ascending, offsets, neighbour ids ascending inside each row)
        self.layers = []
        for l in range(self.nb_layers):
            ids, offs, nbrs = index.get_layer(l).csr()
            offs = offs.astype(np.int64)
            deg = np.diff(offs)
            order = np.lexsort((nbrs, np.repeat(np.arange(len(ids)), deg)))  # (csr() sorts already: not relied on)
            self.layers.append((ids.astype(np.int64), offs, nbrs[order].astype(np.uint32)))

    def sum_levels(self):
        return int(self.levels.sum())

    def header(self, inline, cosine=False):
        fat = self.S0 * self.row_stride if inline else 0
        w = np.zeros(32, dtype=np.uint32)
        w[:18] = [MAGIC, 1, self.kind, self.d, self.n, self.nb_layers, self.ep, self.S0, self.S1, self.row_stride, self.half,
                  4 * (self.d // 8), self.d % 8, fat & 0xFFFFFFFF, fat >> 32, self.m, self.ef_cons, 1 if cosine else 0]
        return w

    def sizes(self, n_lists, n_list_ids, inline):
        return [self.n * self.row_stride, self.n * self.S0 * 4, max(1, self.sum_levels()) * self.S1 * 4, self.n * 4,
                (n_lists + 1) * 4, max(1, n_list_ids) * 4, self.n * self.S0 * self.row_stride if inline else 0]

    def packed_adjacency(self, upper_base):
        """-> (adj0 [N, S0], adj_up [max(1, sum of levels), S1], overflow rows): the in-row part of every row, the last
        slot of a row with more ids than slots left at the bare flag 0x80000000; overflow rows: (0 = adj0 / 1 = adj_up,
        row index, the ids that go to the row's list), layer 0 by id, then the upper rows by row index"""
        ub = np.asarray(upper_base).astype(np.int64)
        adj0 = np.full((self.n, self.S0), EMPTY, dtype=np.uint32)
        adj_up = np.full((max(1, self.sum_levels()), self.S1), EMPTY, dtype=np.uint32)
        over = []
        for l, (ids, offs, nbrs) in enumerate(self.layers):
            out, S = (adj0, self.S0) if l == 0 else (adj_up, self.S1)
            row_of = ids if l == 0 else ub[ids] + l - 1
            deg = np.diff(offs)
            keep = np.where(deg > S, S - 1, deg)
            k_of = np.repeat(np.arange(len(ids)), deg)
            pos = np.arange(len(nbrs)) - np.repeat(offs[:-1], deg)
            sel = pos < keep[k_of]
            out[row_of[k_of[sel]], pos[sel]] = nbrs[sel]
            for k in np.nonzero(deg > S)[0]:
                out[row_of[k], S - 1] = OVF
                over.append((0 if l == 0 else 1, int(row_of[k]), nbrs[offs[k] + S - 1:offs[k + 1]]))
        over.sort(key=lambda t: (t[0], t[1]))
        return adj0, adj_up, over


def upper_base_by_id(levels):
    """a valid upper_base when there is no snapshot to take it from: the ranges handed out in id order"""
    levels = np.asarray(levels).astype(np.int64)
    ub = np.full(len(levels), EMPTY, dtype=np.uint32)
    up = levels > 0
    ub[up] = (np.cumsum(levels[up]) - levels[up]).astype(np.uint32)
    return ub


def validate_upper_base(upper_base, levels, S1, bytes2):
    """a level-0 node holds 0xFFFFFFFF; a node of level L >= 1 a base whose range [base, base + L) is disjoint from every
    other node's; the ranges cover [0, sum of levels); array 2 holds max(1, sum of levels) rows"""
    ub = np.asarray(upper_base).astype(np.int64)
    levels = np.asarray(levels).astype(np.int64)
    if len(ub) != len(levels):
        _fail("upper_base: %d words for %d points", len(ub), len(levels))
    bad = np.nonzero((levels == 0) & (ub != EMPTY))[0]
    if bad.size:
        _fail("upper_base[%d]: a level-0 node holds 0x%08X, not 0xFFFFFFFF", bad[0], ub[bad[0]])
    up = np.nonzero(levels > 0)[0]
    order = up[np.argsort(ub[up], kind="stable")]
    base, L = ub[order], levels[order]
    want = np.cumsum(L) - L
    bad = np.nonzero(base != want)[0]
    if bad.size:
        i = bad[0]
        if i > 0 and base[i] < want[i]:
            _fail("upper_base[%d] = %d: its range [%d, %d) overlaps the range [%d, %d) of node %d", order[i], base[i], base[i],
                  base[i] + L[i], base[i - 1], base[i - 1] + L[i - 1], order[i - 1])
        _fail("upper_base[%d] = %d: the ranges below it end at %d (a gap, or no base at all)", order[i], base[i], want[i])
    total = int(L.sum())
    if bytes2 != max(1, total) * S1 * 4:
        _fail("adj_up: live size %d, expected max(1, %d levels) x %d slots x 4 = %d", bytes2, total, S1,
              max(1, total) * S1 * 4)
    return total


# ---- reading and restating --------------------------------------------------------------------------------------------

class _Mem:  # library-owned device memory for torch (CUDA array interface)
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def read_snapshot(index, device="cuda:0"):
    """the live snapshot, copied out of HBM over exactly desc.bytes[i].  hnsw_snapshot_describe uploads silently when
    the snapshot is stale: the CALLER reads stat("uploads") and stat("patch_fallbacks") around this and asserts that
    they did not move"""
    import torch
    desc = _lib.SnapshotDesc()
    _lib.check(index._L.hnsw_snapshot_describe(index._h, C.byref(desc)))
    torch.cuda.synchronize()
    arrays = []
    for i in range(7):
        nbytes = int(desc.bytes[i])
        if nbytes == 0:
            arrays.append(np.zeros(0, dtype=np.uint8))
            continue
        assert desc.ptr[i], "array %d (%s): %d bytes at a null pointer" % (i, NAMES[i], nbytes)
        arrays.append(torch.as_tensor(_Mem(int(desc.ptr[i]), nbytes), device=device).cpu().numpy().copy())
    return Snapshot(arrays, np.array([desc.header[i] for i in range(32)], dtype=np.uint32))


def expected_snapshot(index, upper_base=None, inline=False, host=None):
    """what a fresh upload of `index` holds, from the host accessors alone.  upper_base: the (validated) array 3 of the
    snapshot under test, None: in id order; inline: whether array 6 exists"""
    g = host if host is not None else Host(index)
    ub = upper_base_by_id(g.levels) if upper_base is None else np.asarray(upper_base, dtype=np.uint32)
    validate_upper_base(ub, g.levels, g.S1, max(1, g.sum_levels()) * g.S1 * 4)
    adj0, adj_up, over = g.packed_adjacency(ub)
    off, lists = [0], []
    for i, (which, row, tail) in enumerate(over):
        (adj0, adj_up)[which][row, -1] = OVF | i
        lists.append(tail)
        off.append(off[-1] + len(tail))
    nbrs = np.concatenate(lists).astype(np.uint32) if lists else np.array([EMPTY], dtype=np.uint32)
    fat = np.zeros(0, dtype=np.uint8)
    if inline:
        fat = inline_blocks(g.rows, adj0, g.half)
    arrays = [g.rows.reshape(-1), adj0, adj_up, ub, np.array(off, dtype=np.uint32), nbrs, fat]
    return Snapshot([np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in arrays], g.header(inline))


def inline_blocks(rows, adj0, half):
    """array 6 from the vector rows and the layer-0 slots: uint8 [N, S0, row_stride]"""
    n, stride = rows.shape
    real = (adj0 != EMPTY) & ((adj0 & OVF) == 0)
    out = u32(rows).reshape(n, stride // 4)[np.where(real, adj0, 0)]  # [N, S0, words]
    out[~real] = 0
    out[:, :, (half - 4) // 4] = adj0
    return out.view(np.uint8).reshape(n, adj0.shape[1], stride)


def split(snap, host):
    """the seven arrays of a snapshot in their shapes: rows u8 [N, row_stride], adj0 u32 [N, S0], adj_up u32 [R, S1],
    upper_base, ovf_off, ovf_nbrs u32, inline u8 [N, S0, row_stride] or None (sizes already checked)"""
    a = snap.arrays
    return (a[0].reshape(host.n, host.row_stride), u32(a[1]).reshape(host.n, host.S0), u32(a[2]).reshape(-1, host.S1), u32(a[3]),
            u32(a[4]), u32(a[5]), a[6].reshape(host.n, host.S0, host.row_stride) if len(a[6]) else None)


def decode_layer(snap, host, layer):
    """(node ids, offsets, neighbour ids) of one layer read out of a snapshot: every row's ids in slot order, then its
    overflow list -- Graph.csr()'s form when the snapshot is canonical"""
    _, adj0, adj_up, ub, off, lst, _ = split(snap, host)
    ids = np.nonzero(host.levels >= layer)[0]
    offs, out = [0], []
    for i in ids:
        row = adj0[i] if layer == 0 else adj_up[int(ub[i]) + layer - 1]
        for x in row:
            if x == EMPTY:
                continue
            if x & OVF:
                li = int(x & ~np.uint32(OVF))
                out.extend(lst[off[li]:off[li + 1]].tolist())
            else:
                out.append(int(x))
        offs.append(len(out))
    return ids.astype(np.uint32), np.array(offs, dtype=np.uint64), np.array(out, dtype=np.uint32)


# ---- the decoded comparison -------------------------------------------------------------------------------------------

def _check_rows(name, a, want, tails, off, lst, n_points, where):
    """a: uint32 [R, S] from the snapshot; want: the host's in-row part of the same rows (bare flag where a list
    follows); tails: {row: the host's ids beyond the row}; where(row) names the row"""
    R, S = a.shape
    n_lists = len(off) - 1
    empty = a == EMPTY
    ptr = ~empty & ((a & OVF) != 0)
    idm = ~empty & ~ptr

    def first(mask):
        r, k = np.argwhere(mask)[0]
        return int(r), int(k)

    hole = empty[:, :-1] & ~empty[:, 1:]
    if hole.any():
        r, k = first(hole)
        _fail("%s %s slot %d: a hole (0xFFFFFFFF) before the word 0x%08X in slot %d", name, where(r), k, a[r, k + 1], k + 1)
    if ptr[:, :-1].any():
        r, k = first(ptr[:, :-1])
        _fail("%s %s slot %d: an overflow pointer 0x%08X outside the last slot", name, where(r), k, a[r, k])
    big = idm & (a >= n_points)
    if big.any():
        r, k = first(big)
        _fail("%s %s slot %d: id %d of %d points", name, where(r), k, a[r, k], n_points)
    down = idm[:, :-1] & idm[:, 1:] & (a[:, 1:] <= a[:, :-1])
    if down.any():
        r, k = first(down)
        _fail("%s %s slot %d: ids not ascending (%d after %d)", name, where(r), k + 1, a[r, k + 1], a[r, k])
    for r in np.nonzero(ptr[:, -1])[0]:
        li = int(a[r, -1] & ~np.uint32(OVF))
        if li >= n_lists:
            _fail("%s %s slot %d: overflow list %d of %d lists", name, where(r), S - 1, li, n_lists)
        tail = lst[off[li]:off[li + 1]]
        if len(tail) == 0:
            _fail("%s %s: its overflow list %d is empty", name, where(r), li)
        if (np.diff(tail.astype(np.int64)) <= 0).any():
            _fail("%s %s: overflow list %d does not ascend: %s", name, where(r), li, tail.tolist())
        if S > 1 and int(tail[0]) <= int(a[r, S - 2]):
            _fail("%s %s: overflow list %d starts at %d, not above the last in-row id %d", name, where(r), li, tail[0],
                  a[r, S - 2])
    # in-row ids + list == the host's sorted neighbour list
    differ = (np.where(ptr, OVF, a) != want)
    if differ.any():
        r, k = first(differ)
        _fail("%s %s slot %d: holds 0x%08X, the host's sorted neighbour list puts 0x%08X there", name, where(r), k, a[r, k],
              want[r, k])
    for r in np.nonzero(ptr[:, -1])[0]:
        li = int(a[r, -1] & ~np.uint32(OVF))
        if not np.array_equal(lst[off[li]:off[li + 1]], tails[int(r)]):
            _fail("%s %s: overflow list %d holds %s, the host's neighbours beyond the row are %s", name, where(r), li,
                  lst[off[li]:off[li + 1]].tolist(), tails[int(r)].tolist())


def check_sizes(snap, host):
    """the live sizes, exactly; -> (number of lists, ids in lists, inline rows present)"""
    got = [len(a) for a in snap.arrays]
    if got[4] < 4 or got[4] % 4:
        _fail("ovf_off: live size %d is not (lists + 1) x 4", got[4])
    n_lists = got[4] // 4 - 1
    n_list_ids = int(u32(snap.arrays[4])[n_lists])
    inline = got[6] != 0
    want = host.sizes(n_lists, n_list_ids, inline)
    for i in range(7):
        if got[i] != want[i]:
            _fail("%s (array %d): live size %d, expected %d", NAMES[i], i, got[i], want[i])
    return n_lists, n_list_ids, inline


def check_header(snap, host, inline):
    want = host.header(inline)
    for i in np.nonzero(snap.header != want)[0]:
        _fail("header word %d (%s): %d, expected %d", i, HEADER_WORDS[i] if i < len(HEADER_WORDS) else "reserved",
              snap.header[i], want[i])


def check_canonical(snap, index, host=None):
    """the snapshot is the canonical form of the index's host graph: raises SnapshotMismatch naming the array, row and
    slot, returns the Host it compared against"""
    g = host if host is not None else Host(index)
    n_lists, n_list_ids, inline = check_sizes(snap, g)
    check_header(snap, g, inline)
    rows, adj0, adj_up, ub, off, lst, fat = split(snap, g)
    validate_upper_base(ub, g.levels, g.S1, len(snap.arrays[2]))
    if off[0] != 0 or (np.diff(off.astype(np.int64)) < 0).any():
        _fail("ovf_off: not ascending from 0: %s", off[:8].tolist())
    if n_lists == 0 and lst[0] != EMPTY:
        _fail("ovf_nbrs: the dummy word of a snapshot without lists holds 0x%08X", lst[0])
    # array 0, byte for byte
    differ = rows != g.rows
    if differ.any():
        r, b = np.argwhere(differ)[0]
        _fail("rows row %d byte %d: holds 0x%02X, expected 0x%02X", r, b, rows[r, b], g.rows[r, b])
    # adjacency
    want0, want_up, over = g.packed_adjacency(ub)
    _check_rows("adj0", adj0, want0, {row: t for which, row, t in over if which == 0}, off, lst, g.n, lambda r: "row %d" % r)
    node_of = np.zeros(len(adj_up), dtype=np.int64)
    layer_of = np.zeros(len(adj_up), dtype=np.int64)
    for i in np.nonzero(g.levels > 0)[0]:
        node_of[int(ub[i]):int(ub[i]) + int(g.levels[i])] = i
        layer_of[int(ub[i]):int(ub[i]) + int(g.levels[i])] = np.arange(1, int(g.levels[i]) + 1)
    _check_rows("adj_up", adj_up, want_up, {row: t for which, row, t in over if which == 1}, off, lst, g.n,
                lambda r: "row %d (node %d, layer %d)" % (r, node_of[r], layer_of[r]))
    # the inline rows: re-derived from arrays 0 and 1 as they stand (both just checked)
    if fat is not None:
        want = inline_blocks(rows, adj0, g.half)
        differ = u32(fat).reshape(g.n, g.S0, -1) != u32(want).reshape(g.n, g.S0, -1)
        if differ.any():
            i, k, w = np.argwhere(differ)[0]
            _fail("inline rows node %d slot %d word %d: holds 0x%08X, expected 0x%08X (adj0[%d][%d] = 0x%08X)", i, k, w,
                  u32(fat).reshape(g.n, g.S0, -1)[i, k, w], u32(want).reshape(g.n, g.S0, -1)[i, k, w], i, k, adj0[i, k])
    return g


def assert_same_bytes(got, want, arrays=range(7), header=True):
    """two snapshots byte for byte; names the array and the row / slot (or byte) of the first difference"""
    if header and not np.array_equal(got.header, want.header):
        i = int(np.nonzero(got.header != want.header)[0][0])
        _fail("header word %d (%s): %d, expected %d", i, HEADER_WORDS[i] if i < len(HEADER_WORDS) else "reserved",
              got.header[i], want.header[i])
    for i in arrays:
        a, b = got.arrays[i], want.arrays[i]
        if len(a) != len(b):
            _fail("%s (array %d): %d bytes, expected %d", NAMES[i], i, len(a), len(b))
        if not np.array_equal(a, b):
            at = int(np.nonzero(a != b)[0][0])
            word = at // 4
            _fail("%s (array %d) byte %d (word %d): holds 0x%08X, expected 0x%08X", NAMES[i], i, at, word,
                  u32(a)[word] if len(a) % 4 == 0 else a[at], u32(b)[word] if len(b) % 4 == 0 else b[at])
