"""The recipes of tests/numeric_range.py do what they claim, and the oracle the GPU is held to is itself right at those
scales (no GPU needed): per fixture and recipe the recipe's condition, on the oracle alone; the oracle's f32 distance
against a numpy float32 left-to-right chain and its 8-bit distance against a numpy float32 restatement of the
reference's eight running sums (host_index.cpp: dist_quant) on the oracle's own codes; the product's host quantiser
against the oracle's; and the selection rule against the matrix."""
import numpy as np
import pytest

import hnsw_rs_amd as H
from oracle import oracle_py as O
from tests import kernel_matrix as KM
from tests import numeric_range as NR
from tests.kernel_matrix import F32, N_POINTS, N_QUERIES, Q8

FIXTURES = sorted({(c.kind, c.d, c.m) for _, c in NR.TABLE + NR.BRUTE_FAST})
fixtures = pytest.mark.parametrize("fx", FIXTURES, ids=lambda f: "%s-d%d-m%d" % ("q8" if f[0] == Q8 else "f32", f[1], f[2]))
recipes = pytest.mark.parametrize("recipe", NR.RECIPES)
f32 = np.float32


def setup(fx, recipe):
    """(oracle, scaled rows, the queries of a 24-query call, product index)"""
    kind, d, m = fx
    vs = KM.fixture(kind, d, m)[2]
    idx, orc, rows, s = NR.fixture(kind, d, m, recipe)
    c = KM.Call(kind, d, m, 0, "batch", 100, 100, N_QUERIES, "default", 0, (), ())
    return orc, rows, NR.queries(c, vs, s), idx


@fixtures
def test_sub_every_squared_sum_is_subnormal_and_not_zero(fx):
    """every brute-force distance of the base queries, the stored rows and the constant row is in (0, 2^-63): its
    square is below 2^-126; the one exception is a stored row's distance to itself"""
    orc, rows, Q, _ = setup(fx, "sub")
    Qs = Q[:N_QUERIES + 3]
    ids, dd = orc.brute_force(Qs, N_POINTS, nthreads=8)
    assert (dd < f32(2.0 ** -63)).all(), dd.max()
    own = {N_QUERIES: 3, N_QUERIES + 1: 777}
    for qi in range(Qs.shape[0]):
        zero = ids[qi][dd[qi] == 0]
        assert zero.tolist() == ([own[qi]] if qi in own else []), (qi, zero)
    assert min(len(set(r.tolist())) for r in dd) > 1000  # (a flushing routine would return one value: 0)


@fixtures
def test_under_every_list_holds_ties(fx):
    orc, rows, Q, _ = setup(fx, "under")
    Qb = Q[:N_QUERIES]
    _, dd, cnt, _ = orc.search_batch(Qb, 100, 100, nthreads=8)
    assert (cnt == 100).all()
    for qi, r in enumerate(dd):
        assert len(set(r.view(np.uint32).tolist())) < 100, qi  # at least one pair of bit-equal distances
    _, da = orc.brute_force(Qb, N_POINTS, nthreads=8)
    assert min(len(set(r.tolist())) for r in da) >= 16


@fixtures
def test_over_most_lists_mix_finite_and_infinite_keys(fx):
    orc, rows, Q, _ = setup(fx, "over")
    _, dd, cnt, _ = orc.search_batch(Q[:N_QUERIES], 100, 100, nthreads=8)
    assert (cnt == 100).all()
    share = np.mean([np.isinf(r).any() and np.isfinite(r).any() for r in dd])
    print("over %r: p = %g, share of mixed lists %.3f" % (fx, NR.OVER_P.get(fx, 0.03), share))
    assert share >= 0.5


def pairs(Q, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, Q.shape[0], 64), rng.integers(0, N_POINTS, 64)


def same_bits(got, want):
    """bit-equal, a NaN for a NaN (the sign and payload of a NaN are not the reference's to define)"""
    got, want = np.asarray(got, dtype=f32), np.asarray(want, dtype=f32)
    return np.array_equal(np.isnan(got), np.isnan(want)) and \
        np.array_equal(got[~np.isnan(want)].view(np.uint32), want[~np.isnan(want)].view(np.uint32))


@recipes
@fixtures
def test_the_oracles_distance_is_the_numpy_chain(fx, recipe):
    """64 (query, row) pairs, the edge queries and (a) .. (e) among them.  f32: t = x - y; s += t * t, left to right,
    sqrt (full.rs:23-29).  8-bit: on the oracle's own codes, x = code * delta + min (two roundings), eight running
    sums over whole chunks, the d % 8 tail into sum 0, the left fold of the eight, sqrt (quant.rs:14-37)."""
    kind, d, m = fx
    orc, rows, Q, _ = setup(fx, recipe)
    qi, ri = pairs(Q, d)
    got = np.array([orc.distance_batch(Q[a], [b])[0] for a, b in zip(qi, ri)], dtype=f32)
    with np.errstate(all="ignore"):
        if kind == F32:
            x, y = rows[ri], Q[qi]
            s = np.zeros(64, dtype=f32)
            for e in range(d):
                t = x[:, e] - y[:, e]
                s = s + t * t
        else:
            def dequant(mn, dl, codes):
                return codes.astype(f32) * f32(dl) + f32(mn)
            x = np.stack([dequant(*orc.get_quant(b)[:3]) for b in ri])
            y = np.stack([dequant(*O.quantize(Q[a])) for a in qi])
            t = x - y
            t2 = t * t
            acc = np.zeros((64, 8), dtype=f32)
            full = d - d % 8
            for c0 in range(0, full, 8):
                acc = acc + t2[:, c0:c0 + 8]
            for e in range(full, d):
                acc[:, 0] = acc[:, 0] + t2[:, e]
            s = np.zeros(64, dtype=f32)
            for j in range(8):
                s = s + acc[:, j]
        want = np.sqrt(s)
    assert want.dtype == f32 and same_bits(got, want), (got[:4], want[:4])
    if recipe == "sub" and kind == F32:
        assert ((s[qi < N_QUERIES] > 0) & (s[qi < N_QUERIES] < f32(2.0 ** -126))).all()  # subnormal, not flushed


@recipes
@pytest.mark.parametrize("fx", [f for f in FIXTURES if f[0] == Q8], ids=lambda f: "q8-d%d-m%d" % f[1:])
def test_the_host_quantiser_is_the_oracles(fx, recipe):
    """codes, min and delta (hnsw_get_quant) of every scaled row; of query (c) (subnormal inputs, under `under` a
    subnormal delta) stored as a point; query (d), whose range overflows to an infinite delta, the product refuses to
    store (include/hnsw_mi355x.h) where the oracle, like the reference, keeps a point that poisons every distance"""
    kind, d, m = fx
    orc, rows, Q, idx = setup(fx, recipe)
    for i in range(N_POINTS):
        g_mn, g_dl, g_codes = idx.get_point(i).quant()
        w_mn, w_dl, w_codes, _ = orc.get_quant(i)
        assert same_bits([g_mn, g_dl], [w_mn, w_dl]) and np.array_equal(g_codes, w_codes), i
    for q in Q[-3:-1]:  # (c), (d)
        w_mn, w_dl, w_codes = O.quantize(q)
        p = H.HNSW.new(m, 32, d, kind)
        if np.isfinite(w_dl):
            p.import_points(q[None], np.zeros(1, dtype=np.uint8))
            g_mn, g_dl, g_codes = p.get_point(0).quant()
            assert same_bits([g_mn, g_dl], [w_mn, w_dl]) and np.array_equal(g_codes, w_codes)
        else:
            with pytest.raises(H.HnswError) as e:
                p.import_points(q[None], np.zeros(1, dtype=np.uint8))
            assert e.value.code == H._lib.ERR_NAN_INPUT
    if recipe == "under":
        assert 0 < O.quantize(Q[-3])[1] < f32(2.0 ** -126)  # (c)'s delta is subnormal


def test_the_selection_covers_every_distance_routine_of_the_matrix():
    """every (kernel family, template arguments but the list width) named by a row of the matrix has a call here,
    and the runner knows its entry point: a new instantiation in the matrix without a range call fails"""
    def routine(k):  # parsed a second way: split at the commas outside nested brackets
        fam, _, rest = k.partition("<")
        args, depth, cur = [], 0, ""
        for ch in rest[:rest.rfind(">")]:
            depth += (ch == "<") - (ch == ">")
            if ch == "," and depth == 0:
                args.append(cur.strip())
                cur = ""
            else:
                cur += ch
        if cur.strip():
            args.append(cur.strip())
        if fam in NR.WIDTH_ARG:
            args.pop(NR.WIDTH_ARG[fam])
        return (fam,) + tuple(args)

    assert routine("hx_lean_f32_kernel<128, Lst<4>, 2>") == ("hx_lean_f32_kernel", "128", "2")
    assert routine("hx_lean_q8_kernel<Lst<1> >") == ("hx_lean_q8_kernel",)
    assert routine("hx_search_kernel<0, 5, 128, 4, true>") == ("hx_search_kernel", "0", "5", "128", "true")
    assert routine("hx_filt_merge_kernel") == ("hx_filt_merge_kernel",)
    want = {routine(k) for row in KM.CASES for k in row.kernels}
    have = {NR.routine_of(k) for kernels, _ in NR.TABLE + NR.BRUTE_FAST for k in kernels}
    assert want == have, (sorted(want - have), sorted(have - want))
    for kernels, c in NR.TABLE + NR.BRUTE_FAST:
        assert c.entry in NR.ENTRIES and c.group in KM.GROUPS, c
    # one call per routine, the ef-100 one where the routine has one
    sel = NR.selection()
    assert len(sel) == len(NR.TABLE) + len(NR.BRUTE_FAST) - len(NR.EXTRA)
    for key, (kernels, c) in sel.items():
        efs = {x.ef for row in KM.CASES if tuple(NR.routine_of(k) for k in row.kernels) == key for x in row.calls}
        assert c.ef == (100 if 100 in efs else min(efs)), (key, c.ef, efs)
    assert len(NR.BRUTE_FAST) == 1
    (k200, c200), = NR.EXTRA
    assert (c200.kind, c200.d, c200.entry, c200.ef) == (F32, 200, "batch", 100) and k200 == ("hx_search_kernel<1, 0, 0, 2, false>",)
