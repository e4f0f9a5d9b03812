"""Diagnostic: per-phase cycle shares of the lean f32 kernel (stamps build).
   HNSW_MI355X_LIB=hnsw_rs_amd/libhnsw_mi355x_stamps.so python scripts/stamps_lean.py [N] [ef ...]
   HX_STAMPS_FRONT=1 with a library built by `make stamps EXTRA=-DHX_STAMPS_FRONT`: the front of the query split further
   (the F_ slots; those stamps lengthen slot 7, so the figures of the two builds do not compare).
   The slots' names, numbers and descriptions are hnsw_rs_amd/csrc/stamp_slots.inc (list LEAN, a merge's split MERGE)."""
import os, sys
sys.path.insert(0, '.')
import numpy as np
import torch
import hnsw_rs_amd as H
from stamp_slots import STRIDE, slots, descriptions
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
efs = [int(x) for x in sys.argv[2:]] or [68]
d, m, nq, n = 100, 16, 1024, 10
vs = H.synth_rows(0, 0x5EED0001, 0, N, d, 32)
idx = H.HNSW.new(m, 32, d, H.VEC_F32)
idx.set_device(0)
idx.insert_bulk_device(vs, 32, False)
qs = H.synth_rows(0, 0x5EED0002, 0, nq, d, 8)
idx.upload()
dev = torch.device('cuda:0')
dQ = torch.from_numpy(qs).to(dev)
ids = torch.empty((nq, n), dtype=torch.int32, device=dev); dd = torch.empty((nq, n), dtype=torch.float32, device=dev)
cnt = torch.empty(nq, dtype=torch.int32, device=dev); st = torch.empty((nq, 4), dtype=torch.int32, device=dev)
FRONT = os.environ.get('HX_STAMPS_FRONT') == '1'
L, M = slots('LEAN'), slots('MERGE')
dbg = torch.zeros((nq, STRIDE), dtype=torch.int64, device=dev)
os.environ['HX_DBG_PTR'] = str(dbg.data_ptr())
names = descriptions('LEAN')
PHASES = ('FRONT', 'PICK', 'FILTER', 'ROW_WAIT', 'CHAIN', 'MERGE_C_ALL', 'IS_P_NEXT', 'COMMIT_P', 'MERGE_P_ALL')
for ef in efs:
    for _ in range(3):
        idx.search_batch_device(dQ.data_ptr(), nq, n, ef, ids.data_ptr(), dd.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0)
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); idx.search_batch_device(dQ.data_ptr(), nq, n, ef, ids.data_ptr(), dd.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0); e1.record()
    torch.cuda.synchronize()
    D = dbg.cpu().numpy().astype(np.float64); S = st.cpu().numpy()
    ms = e0.elapsed_time(e1)
    def C(name, off=None):  # a slot's column; with `off`, a value of the merge split whose base `name` is
        return D[:, L[name] + (M[off] if off else 0)]
    tot = C('TOTAL')
    passes = C('PASSES')
    print('== ef %d: kernel %.4f ms; n_exp %.1f n_dist %.1f layer-0 passes %.1f' % (ef, ms, S[:, 1].mean(), S[:, 0].mean(), passes.mean()))
    print('   max / mean of the per-query cycles: %.3f' % (tot.max() / tot.mean()))
    print('   total cycles per query: mean %.0f p50 %.0f p90 %.0f p99 %.0f max %.0f min %.0f ; implied clock if the max wave spans the kernel: %.2f GHz' % (
        tot.mean(), np.percentile(tot, 50), np.percentile(tot, 90), np.percentile(tot, 99), tot.max(), tot.min(), tot.max() / (ms * 1e6)))
    for nm in PHASES + ('TOTAL',):
        print('   %-45s %9.0f cycles/query %5.1f%%   per pass %7.0f' % (names[L[nm]], C(nm).mean(), 100 * C(nm).mean() / tot.mean(), C(nm).mean() / passes.mean()))
    print('   of slot 7: staging + entry point %.0f cycles/query (the entry point\'s distance is waited for at its end), the walk %.0f' % (
        C('ENTRY').mean(), (C('FRONT') - C('ENTRY')).mean()))
    # the front's own split (the F_ slots, 40 .. 48; its stamps lengthen slot 7): staging alone, the per-layer clear, and per
    # upper-layer expansion the wait for the row it expands, the filter (look, claims), what is left of the row round
    # trip once the filter is done, and the chain; the rest of the walk is the winner, the next row's request, the branches
    if FRONT:
        nx = max(1.0, C('F_EXPANSIONS').mean())
        walk = (C('FRONT') - C('ENTRY')).mean()
        parts = C('F_CLEAR').mean() + C('F_ROW_WAIT').mean() + C('F_FILTER').mean() + C('F_ROWS_LEFT').mean() + C('F_CHAIN').mean()
        print('   front: staging %.0f, entry point %.0f, per-layer clear %.0f cycles/query; %.1f upper expansions, per expansion: wait for the row %.0f, look + claims %.0f, row round trip left %.0f, chain %.0f, winner + next request + rest %.0f; layer-0 table set-up %.0f cycles/query' % (
            C('F_STAGING').mean(), (C('ENTRY') - C('F_STAGING')).mean(), C('F_CLEAR').mean(), C('F_EXPANSIONS').mean(), C('F_ROW_WAIT').mean() / nx, C('F_FILTER').mean() / nx,
            C('F_ROWS_LEFT').mean() / nx, C('F_CHAIN').mean() / nx, (walk - parts) / nx, C('F_TABLE').mean()))
    acc = D[:, [L[nm] for nm in PHASES]].sum(1).mean()
    print('   unaccounted %.1f%%' % (100 * (tot.mean() - acc) / tot.mean()))
    print('   per query: visited slow-loop rounds %.1f; merges with 0 / 1-2 / >=3 survivors: %.1f / %.1f / %.1f; p commits %.1f' % (
        C('SLOW_ROUNDS').mean(), C('MERGES_0').mean(), C('MERGES_1_2').mean(), C('MERGES_3_UP').mean(), C('P_COMMITS').mean()))
    # the merges' own split (slots 26 .. 30 c's merge, 31 .. 35 p's): cycles of the survivor loop, of the LDS phase and of
    # the shift path, the survivors of the big merges, the big merges.  (The split's own stamps lengthen slots 8 and 10.)
    for nm, b in (('merge c', 'MERGE_C'), ('merge p', 'MERGE_P')):
        nbig, nsv = C(b, 'BIG').sum(), C(b, 'SURVIVORS').sum()
        print('   %s: survivor loop %.0f, LDS phase %.0f, shift path %.0f cycles/query; %.1f big merges of %.1f survivors: loop %.0f + LDS phase %.0f cycles per big merge, loop %.1f per survivor' % (
            nm, C(b, 'LOOP').mean(), C(b, 'LDS').mean(), C(b, 'SHIFT').mean(), C(b, 'BIG').mean(), nsv / max(1, nbig),
            C(b, 'LOOP').sum() / max(1, nbig), C(b, 'LDS').sum() / max(1, nbig), C(b, 'LOOP').sum() / max(1, nsv)))
    # the small merges (slots 36 / 37 c's, 38 / 39 p's: merges that took the shift path, the keys they inserted); a small
    # merge holds one or two keys while HX_MERGE_SHIFT_MAX is 2: two-key merges = keys - merges
    for nm, b, c, ck in (('merge c', 'MERGE_C', 'SMALL_C', 'SMALL_C_KEYS'), ('merge p', 'MERGE_P', 'SMALL_P', 'SMALL_P_KEYS')):
        sh, sm, sk = C(b, 'SHIFT'), C(c), C(ck)
        ns, nk = sm.sum(), sk.sum()
        print('   %s: %.1f small merges of %.2f keys per query (with one key %.1f, with more %.1f): shift path %.0f cycles per small merge, %.0f per inserted key' % (
            nm, sm.mean(), nk / max(1, ns), (2 * sm - sk).clip(0).mean(), (sk - sm).clip(None, sm).mean(),
            sh.sum() / max(1, ns), sh.sum() / max(1, nk)))
    # ... and what a merge costs by itself and what every key adds: least squares over the queries
    small, small_keys = C('SMALL_C') + C('SMALL_P'), C('SMALL_C_KEYS') + C('SMALL_P_KEYS')
    shift = C('MERGE_C', 'SHIFT') + C('MERGE_P', 'SHIFT')
    fx, fk = np.linalg.lstsq(np.stack([small, small_keys], axis=1), shift, rcond=None)[0]
    print('   shift path over the queries, least squares: %.0f cycles per small merge + %.0f per inserted key' % (fx, fk))
    # the runner-up's misses: c's merge puts a fresh key below p (slots 16 .. 22)
    miss = C('MISS_1') + C('MISS_2') + C('MISS_3_UP')
    took = C('PASSES_AHEAD')
    print('   per query: misses %.1f, with 1 / 2 / >=3 fresh keys of c below p: %.1f / %.1f / %.1f; follow-up pick is the predicted pair %.2f; follow-up runner-up is the old p %.1f' % (
        miss.mean(), C('MISS_1').mean(), C('MISS_2').mean(), C('MISS_3_UP').mean(), C('MISS_PREDICTED').mean(), C('MISS_OLD_P').mean()))
    # the frontier (its cycles -- inside slot 0, which its own stamp lengthens --, its runs, and the
    # runs after c's merge: a survivor went in front of b, so the pair requested ahead is not the frontier's a and b)
    fr_cyc, fr_runs, fr_again = C('FRONTIER'), C('FRONTIER_RUNS'), C('FRONTIER_RERUNS')
    print('   frontier: %.2f runs per pass, %.0f cycles per run at the pick; %.1f p commits per query, %.1f of them (%.1f%%) took the pair from the pick\'s frontier, %.1f ran it again' % (
        fr_runs.sum() / max(1, passes.sum()), fr_cyc.sum() / max(1, (fr_runs - fr_again).sum()), C('P_COMMITS').mean(),
        (C('P_COMMITS') - fr_again).mean(), 100 * (C('P_COMMITS') - fr_again).sum() / max(1, C('P_COMMITS').sum()), fr_again.mean()))
    print('   pick + adjacency (slot 0) per pass: %.0f cycles on the %.1f passes whose rows were fetched ahead, %.0f on the %.1f others' % (
        C('PICK_AHEAD').sum() / max(1, took.sum()), took.mean(), (C('PICK') - C('PICK_AHEAD')).sum() / max(1, (passes - took).sum()), (passes - took).mean()))
    print('   look + request + claims + chain (slot 1) per pass: %.0f cycles on the %.1f passes whose runner-up kept its distances, %.0f on the %.1f others' % (
        C('FILTER_KEPT').sum() / max(1, C('PASSES_KEPT').sum()), C('PASSES_KEPT').mean(), (C('FILTER') - C('FILTER_KEPT')).sum() / max(1, (passes - C('PASSES_KEPT')).sum()), (passes - C('PASSES_KEPT')).mean()))
    # what do the slowest queries look like?  (the kernel lasts as long as its slowest wave)
    order = np.argsort(-tot)[:8]
    print('   slowest queries: total cycles, n_exp, n_dist, passes, cycles/pass, slow-loop rounds, merges 0/1-2/>=3, p commits')
    for qi in order:
        print('     q%-5d %8.0f  n_exp %4d n_dist %5d passes %4d  %6.0f/pass  slow %3d  merges %3d/%3d/%3d  pcommits %3d' % (
            qi, tot[qi], S[qi, 1], S[qi, 0], passes[qi], tot[qi] / max(1, passes[qi]), C('SLOW_ROUNDS')[qi], C('MERGES_0')[qi], C('MERGES_1_2')[qi], C('MERGES_3_UP')[qi], C('P_COMMITS')[qi]))
        print('            misses 1/2/>=3 below p %3d/%3d/%3d  predicted %3d  old p again %3d  slot 0 per pass: ahead %5.0f (%3d passes), others %5.0f  slot 1 per pass %5.0f  kept %3d passes at %5.0f' % (
            C('MISS_1')[qi], C('MISS_2')[qi], C('MISS_3_UP')[qi], C('MISS_PREDICTED')[qi], C('MISS_OLD_P')[qi], C('PICK_AHEAD')[qi] / max(1, took[qi]), took[qi],
            (C('PICK')[qi] - C('PICK_AHEAD')[qi]) / max(1, passes[qi] - took[qi]), C('FILTER')[qi] / max(1, passes[qi]), C('PASSES_KEPT')[qi], C('FILTER_KEPT')[qi] / max(1, C('PASSES_KEPT')[qi])))
        print('            merge c + p: survivor loop %6.0f  LDS phase %6.0f  shift path %6.0f cycles; big merges %3d with %4d survivors' % tuple(
            (C('MERGE_C', o) + C('MERGE_P', o))[qi] for o in ('LOOP', 'LDS', 'SHIFT', 'BIG', 'SURVIVORS')))
        print('            small merges %3d with %3d keys: shift path %5.0f cycles per small merge, %5.0f per key, %.1f%% of the query' % (
            small[qi], small_keys[qi], shift[qi] / max(1, small[qi]), shift[qi] / max(1, small_keys[qi]), 100 * shift[qi] / tot[qi]))
    cc = np.corrcoef(tot, S[:, 1])[0, 1]
    fit = np.polyfit(S[:, 1].astype(np.float64), tot, 1)
    print('   corr(total cycles, n_exp) = %.3f; fit: cycles = %.0f * n_exp + %.0f; n_exp mean %.1f p99 %.0f max %d' % (
        cc, fit[0], fit[1], S[:, 1].mean(), np.percentile(S[:, 1], 99), S[:, 1].max()))
    res = tot - np.polyval(fit, S[:, 1].astype(np.float64))
    print('   residual of that fit: std %.0f, max %.0f, min %.0f' % (res.std(), res.max(), res.min()))
