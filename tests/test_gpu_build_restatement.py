"""The on-device build ("gpu_build" = 2, hnsw_insert_bulk_device) edge for edge against its CPU restatement
(oracle/batched_build.cpp, OracleHNSW.insert_bulk_batched).  The device build is deterministic for a given batch
schedule ("Order and batching"), so its exact graph is defined: same entry point, same layers, same node
ids and the same neighbour set in every row.  Recall thresholds and graph invariants cannot see a near-tie pruned the
wrong way or a kept-last-edge mirrored on the wrong side; this can.  The cases reach every kernel instantiation the
device-connect build launches (CASES).  Every test here needs a real MI355X."""
import numpy as np
import pytest

import hnsw_rs_amd as H
from oracle import oracle_py as O
from tests.util import graph_difference

pytestmark = pytest.mark.gpu

NTHREADS = 8  # the restatement's phase-1 threads (a GPU job has 16 CPUs)


def build_both(vs, lv, m, ef_cons, kind, batch=None, base=None, base_threads=1):
    """(product index, oracle index, restatement counts): `base` rows (with their levels) first on the CPU -- the
    product's single-thread build is the oracle's insert_bulk -- then the rest on the device / restated"""
    d = vs.shape[1]
    idx = H.HNSW.new(m, ef_cons, d, kind)
    orc = O.OracleHNSW(m, ef_cons, d, kind)
    start = 0
    if base is not None:
        start = base
        idx.insert_bulk(vs[:base], base_threads, False, levels=lv[:base])
        orc.insert_bulk(vs[:base], lv[:base])
    bmax, bdiv = batch if batch is not None else (8192, 8)
    if batch is not None:
        idx.set_option("gpu_build_batch_max", bmax)
        idx.set_option("gpu_build_batch_div", bdiv)
    idx.insert_bulk_device(vs[start:], 8, False, levels=lv[start:])
    st = orc.insert_bulk_batched(vs[start:], lv[start:], batch_max=bmax, batch_div=bdiv, nthreads=NTHREADS)
    return idx, orc, st


def check_same(idx, orc, st, what):
    assert idx.stat("build_cpu_path_points") == 0, what
    assert idx.stat("build_batches") == st["batches"], (what, idx.stat("build_batches"), st)
    diff = graph_difference(idx, orc)
    assert diff is None, "%s: %s" % (what, diff)
    assert idx.stat("build_kept_last_edges") == st["kept_last_edges"], (what, idx.stat("build_kept_last_edges"), st)


def I(kind, ds):
    return "hx_insert_kernel<%d, %d>" % (kind, ds)


def C(kind, ds, rs):
    return "hx_connect_kernel<%d, %d, %d>" % (kind, ds, rs)


Q8, F32 = H.VEC_QUANT8, H.VEC_F32
REMOVE = {1: "hx_remove_kernel<1>", 2: "hx_remove_kernel<2>", 4: "hx_remove_kernel<4>"}

# (kind, d, m, ef_cons, n, kernels): every hx_insert_kernel<KIND, DS> that launch_insert picks (d = 100, 128, 256, 768
# and the generic DS = 0, both kinds), every hx_connect_kernel<KIND, DS, RS> (RS = 1 at d = 100, 128, 256, 768 and
# generic; RS = 2 / 4 -- m = 64 / 128 -- generic, both kinds) and hx_remove_kernel<1 / 2 / 4>.  `kernels` names the
# insert and connect instantiations the build must launch (the kernel log holds exactly these of the two templates)
# and the remove instantiation it may launch
CASES = [
    pytest.param(Q8, 100, 16, 32, 20000, (I(Q8, 100), C(Q8, 100, 1), REMOVE[1]), id="quant8-d100-default-schedule"),
    pytest.param(F32, 100, 16, 32, 20000, (I(F32, 100), C(F32, 100, 1), REMOVE[1]), id="f32-d100-default-schedule"),
    pytest.param(Q8, 128, 16, 32, 4000, (I(Q8, 128), C(Q8, 128, 1), REMOVE[1]), id="quant8-d128"),
    pytest.param(Q8, 256, 16, 32, 4000, (I(Q8, 256), C(Q8, 256, 1), REMOVE[1]), id="quant8-d256"),
    pytest.param(Q8, 768, 16, 32, 4000, (I(Q8, 768), C(Q8, 768, 1), REMOVE[1]), id="quant8-d768"),
    pytest.param(F32, 128, 16, 32, 5000, (I(F32, 128), C(F32, 128, 1), REMOVE[1]), id="f32-d128-coop-rows"),
    pytest.param(F32, 256, 16, 32, 5000, (I(F32, 256), C(F32, 0, 1), REMOVE[1]), id="f32-d256-row-stride-1024"),
    pytest.param(F32, 768, 16, 32, 5000, (I(F32, 768), C(F32, 0, 1), REMOVE[1]), id="f32-d768-row-stride-3072"),
    pytest.param(F32, 33, 16, 32, 6000, (I(F32, 0), C(F32, 0, 1), REMOVE[1]), id="f32-d33-generic"),
    pytest.param(Q8, 60, 16, 32, 6000, (I(Q8, 0), C(Q8, 0, 1), REMOVE[1]), id="quant8-d60-generic"),
    pytest.param(Q8, 100, 24, 48, 8000, (I(Q8, 100), C(Q8, 100, 1), REMOVE[1]), id="m24-64-slot-rows"),
    pytest.param(F32, 48, 64, 48, 5000, (I(F32, 0), C(F32, 0, 2), REMOVE[2]), id="f32-m64-128-slot-rows"),
    pytest.param(Q8, 48, 64, 48, 5000, (I(Q8, 0), C(Q8, 0, 2), REMOVE[2]), id="quant8-m64-128-slot-rows"),
    pytest.param(F32, 60, 128, 48, 4000, (I(F32, 0), C(F32, 0, 4), REMOVE[4]), id="f32-m128-256-slot-rows"),
    pytest.param(Q8, 60, 128, 48, 4000, (I(Q8, 0), C(Q8, 0, 4), REMOVE[4]), id="quant8-m128-256-slot-rows"),
    pytest.param(Q8, 100, 16, 100, 6000, (I(Q8, 100), C(Q8, 100, 1), REMOVE[1]), id="ef100-table-2-13"),
    pytest.param(F32, 64, 16, 200, 6000, (I(F32, 0), C(F32, 0, 1), REMOVE[1]), id="ef200-table-2-14"),
]
# what these cases launch, for tests/test_kernel_matrix_complete.py
BUILD_KERNELS = sorted({k for c in CASES for k in c.values[5]})


def check_kernels(log, kernels, what):
    """the insert and connect instantiations are exactly `kernels`' ones, a remove (if any) is `kernels`' one"""
    got = {k for k in log if k.startswith(("hx_insert_kernel<", "hx_connect_kernel<"))}
    want = {k for k in kernels if not k.startswith("hx_remove_kernel<")}
    assert got == want, (what, dict(log))
    removes = {k for k in log if k.startswith("hx_remove_kernel<")}
    assert removes <= set(kernels), (what, dict(log))


@pytest.mark.parametrize("kind,d,m,ef_cons,n,kernels", CASES)
def test_device_build_equals_the_restatement(kind, d, m, ef_cons, n, kernels):
    vs = H.synth_rows(0, 0xB17D0000 + d * 1000 + m, 0, n, d)
    lv = O.draw_levels(n, m, 0xB17D + m)
    with H.kernel_log() as log:
        idx, orc, st = build_both(vs, lv, m, ef_cons, kind)
    check_kernels(log, kernels, "kind=%d d=%d m=%d" % (kind, d, m))
    # phase 1 reached the heuristic's special paths: a candidate set cut to its 512 nearest, and more than 128
    # candidates popped (the kernel's sweep window grows past its first 128)
    assert st["batches"] > 0 and st["heuristic_cut"] > 0 and st["heuristic_past_window"] > 0, st
    check_same(idx, orc, st, "kind=%d d=%d m=%d ef=%d" % (kind, d, m, ef_cons))


@pytest.mark.parametrize("kind", [H.VEC_F32, H.VEC_QUANT8])
def test_exact_ties_are_broken_by_id(kind):
    """coordinates in {0, 1, 2, 3}: distances are square roots of small integers, so nearly every comparison of the
    searches, the heuristic and the prunes ties on distance, and some points are duplicates (distance 0).  Every
    such tie is decided by id; a kernel that broke one the other way builds a different graph"""
    n, d, m = 6000, 8, 16
    vs = np.random.Generator(np.random.PCG64(0xB17D7)).integers(0, 4, (n, d)).astype(np.float32)
    lv = O.draw_levels(n, m, 0xB17D8)
    idx, orc, st = build_both(vs, lv, m, 32, kind)
    check_same(idx, orc, st, "ties, kind=%d" % kind)


def test_small_m_clamps_the_seed_and_mirrors_kept_last_edges():
    """m = 5 (16-slot rows, cap 10 / 5): the sequential seed leaves rows over the cap, so
    clamp_rows_to_cap drops edges and restores the ones that were the other side's last; the drop kernel refuses
    last edges too.  Both must be mirrored exactly as the restatement does"""
    n, d, m = 8000, 100, 5
    vs = H.synth_rows(0, 0xB17D0005, 0, n, d)
    lv = O.draw_levels(n, m, 0xB17D05)
    idx, orc, st = build_both(vs, lv, m, 32, H.VEC_QUANT8)
    # both sources of kept-last-edges: the clamp's restores and phase 3's refusals
    assert 0 < st["clamp_restores"] < st["kept_last_edges"], st
    check_same(idx, orc, st, "m=5")


@pytest.mark.parametrize("batch", [(64, 64), (32768, 2)], ids=["batches-64", "batches-32768-div2"])
def test_batch_schedules_equal_the_restatement(batch):
    """the batch-size rule at both ends: 64-point batches, and 1 / 2 of the connected points (up to 32768)"""
    n, d, m = 40000, 32, 16
    vs = H.synth_rows(0, 0xB17D0040, 0, n, d)
    lv = O.draw_levels(n, m, 0xB17D40)
    idx, orc, st = build_both(vs, lv, m, 32, H.VEC_F32, batch=batch)
    check_same(idx, orc, st, "schedule %s" % (batch,))


@pytest.mark.parametrize("base", [5000, 1000], ids=["no-seed", "partial-seed"])
def test_extension_equals_the_restatement(base):
    """an index that already holds points (built on the CPU, one thread: the oracle's graph) extended on the device:
    with 5000 points there is no seed and the clamp runs on the CPU-built graph; with 1000 the seed is partial"""
    n, d, m = base + (7000 if base == 5000 else 11000), 100, 16
    vs = H.synth_rows(0, 0xB17D0100 + base, 0, n, d)
    lv = O.draw_levels(n, m, 0xB17D100 + base)
    # a later point above the current top layer would become an entry point that is never connected (the
    # reference's own TODO, template.rs:283-290): keep the levels below it
    lv[base:] = np.minimum(lv[base:], lv[:base].max())
    idx, orc, st = build_both(vs, lv, m, 32, H.VEC_QUANT8, base=base)
    assert st["seed_points"] == max(0, 2048 - base)
    check_same(idx, orc, st, "extension of %d" % base)


def test_rerun_with_a_larger_visited_table_equals_the_restatement(monkeypatch):
    """HNSW_MI355X_INSERT_TABLE_ADJUST=-3: the first launch of every batch gets an eighth of the visited table, the
    points that fill it run again with a larger one -- a search's result does not depend on the table's size"""
    monkeypatch.setenv("HNSW_MI355X_INSERT_TABLE_ADJUST", "-3")
    n, d, m = 8000, 100, 16
    vs = H.synth_rows(0, 0xB17D0200, 0, n, d)
    lv = O.draw_levels(n, m, 0xB17D200)
    idx, orc, st = build_both(vs, lv, m, 64, H.VEC_F32)
    assert idx.stat("build_rerun_points") > 0
    check_same(idx, orc, st, "table adjust -3")
