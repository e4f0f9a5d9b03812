"""No GPU: the fixtures of tests/upper_walk.py do what their names promise (a CPU replay over the oracle's
search_layer: the winner of every layer, the improvements on it, the row taken on every descent), so that a fixture
that stops provoking its path fails here; and the lean kernels whose upper-layer walk requests its rows ahead still
fit two waves per SIMD (the method of tests/test_kernel_resources.py: hipcc cross-compiles for gfx950 and reports each
kernel's registers)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import upper_walk as UW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


KINDS = (UW.F32, UW.QUANT8)
KIND_ID = {UW.F32: "f32", UW.QUANT8: "quant8"}.get


@pytest.mark.parametrize("name", sorted(UW.CASES))
@pytest.mark.parametrize("kind", KINDS, ids=KIND_ID)
def test_case_has_its_pattern(kind, name):
    got = UW.assert_pattern(name, kind)
    c, orc = UW.fixture(name, kind)
    assert orc.nb_layers == int(c.levels.max()) + 1 and len(got) == orc.nb_layers - 1
    assert len(c.queries) <= 16


def test_pools_are_ordered():
    """every step is strictly nearer to q* than the steps before it, every filler farther than every step, the decoy
    nearer than all of them: what the cases' rows rest on"""
    c = UW.Case("pools")
    d = UW.distances(c.rows, c.queries[0])
    steps = [c.step(0) for _ in range(30)]
    fill = [c.filler(0) for _ in range(120)]
    dz = c.decoy(0)
    assert all(d[a] > d[b] for a, b in zip(steps, steps[1:]))
    assert min(d[fill]) > d[steps[0]] and d[dz] < d[steps[-1]]


def test_tower_descends_on_rows_of_its_own():
    """five descents in a row and no improvement: the rows differ in degree, so a row taken from the wrong layer shows
    in sum_deg"""
    c, orc = UW.fixture("tower")
    degs = [len(orc.neighbors(l, c.ep)) for l in range(5, -1, -1)]
    assert degs == [6, 5, 4, 3, 2, 8]
    assert orc.nb_layers == 6 and int(c.levels[c.ep]) == 5


def test_stairs_exact_takes_a_whole_layer0_row():
    c, orc = UW.fixture("stairs_exact")
    w1 = c.expect[-1][1]
    row = c.adj0[w1]
    assert int(c.levels[w1]) == 1 and len(row) == UW.S0
    d = orc.distance_batch(c.queries[0], np.array(row, dtype=np.uint32))
    assert d[16:].max() < d[:16].min()  # the nearer half sits behind slot 16


def test_runs_replaces_the_row_below():
    c, orc = UW.fixture("runs")
    assert [e[2] for e in c.expect] == [1, 2, 7]
    decoy = c.order[UW.N - 1]  # the nearest id to q*
    # every node the walk leaves by an improvement holds the decoy alone one layer down
    left = [n for l in (3, 2, 1) for n, r in c.up[l].items() if len(r) == 3]
    assert len(left) == 10
    for l in (3, 2, 1):
        for n, r in c.up[l].items():
            if len(r) == 3:
                below = c.up[l - 1][n] if l > 1 else c.adj0[n]
                assert below == [decoy], (l, n, below)


@pytest.mark.parametrize("name", sorted(UW.REFUSED))
@pytest.mark.parametrize("kind", KINDS, ids=KIND_ID)
def test_reference_refuses_every_query(kind, name):
    UW.assert_refused(name, kind)


def test_product_import_refuses_a_neighbour_below_its_layer():
    """level0_neighbour cannot reach a kernel: import_layer answers HNSW_ERR_NODE_NOT_IN_GRAPH for the row that lists
    the node of level 0 (level0_entry is the part of the case an index can hold)"""
    import hnsw_rs_amd as H
    with pytest.raises(H.HnswError) as e:
        UW.product("level0_neighbour")
    assert e.value.code == H._lib.ERR_NODE_NOT_IN_GRAPH
    assert int(UW.product("level0_entry").params.ep) == UW.fixture("level0_entry")[0].ep


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_walk_ahead_kernels_fit_two_waves_per_simd(tmp_path):
    src = os.path.join(ROOT, "hnsw_rs_amd", "csrc", "search_lean.hip")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
           "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "lean.o"),
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
    # <100, Lst<1>> and <100, LstHT> of the f32 kernel, Lst<1> and LstHT of the quant8 kernel
    want = [r"hx_lean_f32_kernelILi100ENS0_3LstILi1EEE", r"hx_lean_f32_kernelILi100ENS0_5LstHTE",
            r"hx_lean_q8_kernelINS0_3LstILi1EEE", r"hx_lean_q8_kernelINS0_5LstHTE"]
    for pat in want:
        hit = [k for k in kernels if re.search(pat, k)]
        assert len(hit) == 1, (pat, sorted(kernels))
        r = kernels[hit[0]]
        assert r.get("VGPRs", 999) <= 248 and r.get("AGPRs", 0) == 0, (hit[0], r)
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (hit[0], r)
        assert r.get("Occupancy", 0) >= 2, (hit[0], r)
