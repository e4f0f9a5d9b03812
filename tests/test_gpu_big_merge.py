"""The lean kernels' big merge (search_lean.hip, DESIGN.md 4a: three or more survivors are compacted into LDS, read
back by broadcast to rank them against the list, the list scattered and the holes filled) against the CPU oracle,
through the C ABI: ids, distance bits, counts and the three counters, and the kernel that is expected ran.  The
fixtures are tests/big_merge.py's; every hand-made graph first proves on the CPU replay that it provokes the merges its
names promise (the assertions of tests/test_big_merge_host.py).  f32 rows at d = 100 over lists of one register, head +
tail and four registers; 8-bit rows at d = 100; f32 rows at d = 128, whose gather's stage image shares the merge's LDS."""
import pytest

import hnsw_rs_amd as H
from oracle import oracle_py as O
from tests import big_merge as BM
from tests import runner_up_miss as RM
from tests.util import assert_search_equal, product_from_oracle

pytestmark = pytest.mark.gpu

_INDEX = {}


def lst_of(ef):
    return "Lst<1>" if ef <= 64 else ("LstHT" if ef <= 128 else "Lst<4>")


def kernel_of(kind, dim, ef):
    lst = lst_of(ef)
    if kind == O.VEC_QUANT8:
        return "hx_lean_q8_kernel<%s>" % (lst + " " if lst.endswith(">") else lst)
    return "hx_lean_f32_kernel<%d, %s, 4>" % (dim, lst)


def run(index, orc, qs, ef, kernel, what):
    with H.kernel_log() as log:
        got = index.search_batch(qs, BM.TOPN, ef)
    assert kernel in log, (what, kernel, dict(log))
    assert_search_equal(got, orc.search_batch(qs, BM.TOPN, ef, nthreads=8), what)


def handmade(key, dim, kind):
    orc, rows, lv, qs, _ = BM.handmade(key, dim, kind)
    if (key, dim, kind) not in _INDEX:
        _INDEX[(key, dim, kind)] = product_from_oracle(orc, rows, lv)
    return _INDEX[(key, dim, kind)], orc, qs


@pytest.mark.parametrize("ef", BM.EFS)
@pytest.mark.parametrize("key", BM.BUILDERS)
def test_f32_100d(key, ef):
    for name, (k, _, efs) in BM.GRAPHS.items():
        if k == key and ef in efs:
            BM.assert_pattern(name, ef, BM.replayed(key, ef)[2])
    index, orc, qs = handmade(key, 100, O.VEC_F32)
    run(index, orc, qs, ef, kernel_of(O.VEC_F32, 100, ef), "%s f32 100d ef=%d" % (key, ef))


@pytest.mark.parametrize("ef", (64, 68))
@pytest.mark.parametrize("key", BM.BUILDERS)
def test_quant8_100d(key, ef):
    index, orc, qs = handmade(key, 100, O.VEC_QUANT8)
    run(index, orc, qs, ef, kernel_of(O.VEC_QUANT8, 100, ef), "%s quant8 100d ef=%d" % (key, ef))


@pytest.mark.parametrize("key", BM.BUILDERS)
def test_f32_128d(key):
    index, orc, qs = handmade(key, 128, O.VEC_F32)
    run(index, orc, qs, 68, kernel_of(O.VEC_F32, 128, 68), "%s f32 128d ef=68" % key)


@pytest.fixture(scope="module")
def built():
    orc, vs, lv, qs = RM.built()
    return product_from_oracle(orc, vs, lv), orc, qs


@pytest.mark.parametrize("ef", RM.EFS)
def test_built_index(built, ef):
    index, orc, qs = built
    run(index, orc, qs, ef, kernel_of(O.VEC_F32, 100, ef), "built ef=%d" % ef)
