"""The on-device build under "rows_f16" (build_kernels16.hip): over X it builds, edge for edge, the
graph the CPU restatement (OracleHNSW.insert_bulk_batched) makes over X16 = X.astype(float16).astype(float32), from
binary16 rows in HBM, and the snapshot it leaves is the f16 one the next search reads.  CASES names every kernel of
libhnsw_mi355x_build16.so (tests/test_build_rows_f16_host.py).  Every test needs an MI355X; on a library that builds from
an f32 snapshot the first three fail on the kernel log and the last on `uploads`."""
import numpy as np
import pytest

import hnsw_rs_amd as H
from oracle import oracle_py as O
from tests.test_gpu_build_restatement import NTHREADS, check_same
from tests.util import assert_search_equal

pytestmark = pytest.mark.gpu


def widen(X):
    return X.astype(np.float16).astype(np.float32)


def build_both(X, lv, m, ef_cons, base=0):
    """(index under the option over X, restatement over X16, its counts, the kernel log): `base` rows on the CPU first"""
    d = X.shape[1]
    idx = H.HNSW.new(m, ef_cons, d, H.VEC_F32)
    idx.set_option("rows_f16", 1)
    orc = O.OracleHNSW(m, ef_cons, d, H.VEC_F32)
    X16 = widen(X)
    if base:
        idx.insert_bulk(X[:base], 1, False, levels=lv[:base])
        orc.insert_bulk(X16[:base], lv[:base])
    with H.kernel_log() as log:
        idx.insert_bulk_device(X[base:], 8, False, levels=lv[base:])
    st = orc.insert_bulk_batched(X16[base:], lv[base:], batch_max=8192, batch_div=8, nthreads=NTHREADS)
    return idx, orc, st, log


def check_kernels(log, ds, rs):
    got = {k for k in log if k.startswith(("hx_insert", "hx_connect"))}
    assert got == {"hx_insert16_kernel<%d>" % ds, "hx_connect16_kernel<%d>" % rs}, dict(log)


# (d, m, ef_cons, n, DS, RS): the four insert and three connect instantiations, both gather rounds (d = 128 / 256 / 768:
# whole row in flight, ring exactly full, ring refilled), the lane-per-row tails (d = 100: 13 pieces, tail of 4; 33: tail of
# 1; 6: one padded piece; 64: exactly one stage), the 2^14-slot table, and rows too wide for the two-entry pass
CASES = [(128, 16, 32, 5000, 128, 1), (256, 16, 32, 5000, 256, 1), (768, 16, 32, 5000, 768, 1), (100, 16, 32, 6000, 0, 1),
         (33, 16, 32, 6000, 0, 1), (6, 16, 32, 6000, 0, 1), (64, 16, 200, 6000, 0, 1), (48, 64, 32, 5000, 0, 2),
         (60, 128, 32, 4000, 0, 4)]


@pytest.mark.parametrize("d,m,ef_cons,n,ds,rs", CASES)
def test_device_build_from_f16_rows_equals_the_restatement(d, m, ef_cons, n, ds, rs):
    X = H.synth_rows(0, 0xB16D0000 + d * 1000 + m, 0, n, d)
    lv = O.draw_levels(n, m, 0xB16D + m)
    idx, orc, st, log = build_both(X, lv, m, ef_cons)
    check_kernels(log, ds, rs)
    # phase 1 reached the heuristic's special paths, as in the f32 test.  At d = 6 neighbourhoods overlap so much that no
    # candidate set reaches 512 (the restatement over X16 cuts none at n = 6000 .. 48000): only the window is asserted there
    assert st["batches"] > 0 and (st["heuristic_cut"] > 0 or d == 6) and st["heuristic_past_window"] > 0, st
    check_same(idx, orc, st, "d=%d m=%d ef=%d" % (d, m, ef_cons))


def test_exact_ties_are_broken_by_id():
    """coordinates in {0..3}, exact in binary16: nearly every comparison ties on distance and is decided by id"""
    n, d, m = 6000, 8, 16
    X = np.random.Generator(np.random.PCG64(0xB16D7)).integers(0, 4, (n, d)).astype(np.float32)
    idx, orc, st, log = build_both(X, O.draw_levels(n, m, 0xB16D8), m, 32)
    check_kernels(log, 0, 1)
    check_same(idx, orc, st, "ties")


def test_extension_evaluates_the_edges_that_predate_the_build():
    """5000 points built on the CPU, 7000 more on the device: the base's edges carry no stored distance, so
    hx_connect16_kernel<1> stages the node's row and evaluates them with a lane per row"""
    base, n, d, m = 5000, 12000, 100, 16
    X = H.synth_rows(0, 0xB16D0100, 0, n, d)
    lv = O.draw_levels(n, m, 0xB16D100)
    lv[base:] = np.minimum(lv[base:], lv[:base].max())  # (no later point above the top layer: template.rs:283-290)
    idx, orc, st, log = build_both(X, lv, m, 32, base=base)
    check_kernels(log, 0, 1)
    assert st["seed_points"] == 0
    check_same(idx, orc, st, "extension")


@pytest.mark.parametrize("d", [100, 128])
def test_the_snapshot_kept_is_the_f16_one(d):
    n, m = 5000, 16
    X = H.synth_rows(0, 0xB16D0200 + d, 0, n, d)
    Q = H.synth_rows(0, 0xB16D0300 + d, 0, 40, d)
    lv = O.draw_levels(n, m, 0xB16D200)
    idx = H.HNSW.new(m, 32, d, H.VEC_F32)
    idx.set_option("rows_f16", 1)
    plain = H.HNSW.new(m, 32, d, H.VEC_F32)
    idx.insert_bulk_device(X, 8, False, levels=lv), plain.insert_bulk_device(widen(X), 8, False, levels=lv)
    got, want = idx.search_batch(Q, 10, 64), plain.search_batch(Q, 10, 64)
    assert idx.stat("uploads") == plain.stat("uploads")
    saved = n * (((4 * d + 15) & ~15) - 16 * -(-2 * d // 16))
    assert saved > 0 and idx.stat("snapshot_bytes") == plain.stat("snapshot_bytes") - saved
    assert_search_equal(got, want, "d=%d" % d)
