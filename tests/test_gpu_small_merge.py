"""The lean kernels' small merge (search_lean.hip, DESIGN.md 4a: one or two survivors are inserted by shifting the list
-- compare masks and selects, the head's last entry carried to the tail's front, one cut and one bound behind the last
key) against the CPU oracle, through the C ABI: ids, distance bits, counts and the three counters, and the kernel that
is expected ran.  The fixtures are tests/small_merge.py's, one hand-made graph per ef; every graph first proves on the
CPU replay that its rows provoke the merges their names promise (the assertions of tests/test_small_merge_host.py).
f32 rows at d = 100 and 8-bit rows at d = 100 over lists of one register, head + tail and four registers; f32 rows at
d = 128, whose gather's stage image shares the merge's LDS, at ef 68 and 256."""
import pytest

import hnsw_rs_amd as H
from oracle import oracle_py as O
from tests import small_merge as SM
from tests.util import assert_search_equal, product_from_oracle

pytestmark = pytest.mark.gpu


def lst_of(ef):
    return "Lst<1>" if ef <= 64 else ("LstHT" if ef <= 128 else "Lst<4>")


def kernel_of(kind, dim, ef):
    lst = lst_of(ef)
    if kind == O.VEC_QUANT8:
        return "hx_lean_q8_kernel<%s>" % (lst + " " if lst.endswith(">") else lst)
    # d = 128, a launch of at most one wave per SIMD: the four-stage gather up to two list registers, two stages beyond
    return "hx_lean_f32_kernel<%d, %s, %d>" % (dim, lst, 4 if dim == 100 or ef <= 128 else 2)


def run(ef, dim, kind, what):
    orc, rows, lv, qs, s = SM.handmade(ef, dim, kind)
    index = product_from_oracle(orc, rows, lv)
    kernel = kernel_of(kind, dim, ef)
    with H.kernel_log() as log:
        got = index.search_batch(qs, SM.TOPN, ef)
    assert kernel in log, (what, kernel, dict(log))
    assert_search_equal(got, orc.search_batch(qs, SM.TOPN, ef, nthreads=8), what)


@pytest.mark.parametrize("ef", SM.EFS)
def test_f32_100d(ef):
    SM.assert_pattern(ef, SM.replayed(ef)[2], SM.script(ef))
    run(ef, 100, O.VEC_F32, "small merge f32 100d ef=%d" % ef)


@pytest.mark.parametrize("ef", SM.EFS)
def test_quant8_100d(ef):
    run(ef, 100, O.VEC_QUANT8, "small merge quant8 100d ef=%d" % ef)


@pytest.mark.parametrize("ef", (68, 256))
def test_f32_128d(ef):
    run(ef, 128, O.VEC_F32, "small merge f32 128d ef=%d" % ef)
