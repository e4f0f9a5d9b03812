"""Diagnostic: per-phase cycle shares of the lean f32 kernel (stamps build).
   HNSW_MI355X_LIB=hnsw_rs_amd/libhnsw_mi355x_stamps.so python scripts/stamps_lean.py [N] [ef ...]
   HX_STAMPS_FRONT=1 with a library built by `make stamps EXTRA=-DHX_STAMPS_FRONT`: the front of the query split further
   (50 values per query instead of 40; those stamps lengthen slot 7, so the figures of the two builds do not compare)."""
import os, sys
sys.path.insert(0, '.')
import numpy as np
import torch
import hnsw_rs_amd as H
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
SLOTS = 53 if FRONT else 43  # HX_LEAN_DBG_SLOTS (search_lean.hip)
dbg = torch.zeros((nq, SLOTS), dtype=torch.int64, device=dev)
os.environ['HX_DBG_PTR'] = str(dbg.data_ptr())
names = {0: 'pick c,p + adjacency row round trip', 1: 'visited: insert c, look up p', 2: 'row gather until landed',
         3: 'chain + sqrt + key', 8: 'merge c', 9: 'overflow rows + pick + is-p-next', 5: 'commit p: mark + visited insert',
         10: 'commit p: merge + pick', 7: 'staging + entry + upper layers', 4: 'TOTAL (whole query)'}
for ef in efs:
    for _ in range(3):
        idx.search_batch_device(dQ.data_ptr(), nq, n, ef, ids.data_ptr(), dd.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0)
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); idx.search_batch_device(dQ.data_ptr(), nq, n, ef, ids.data_ptr(), dd.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0); e1.record()
    torch.cuda.synchronize()
    D = dbg.cpu().numpy().astype(np.float64); S = st.cpu().numpy()
    ms = e0.elapsed_time(e1)
    tot = D[:, 4]
    passes = D[:, 6]
    print('== ef %d: kernel %.4f ms; n_exp %.1f n_dist %.1f layer-0 passes %.1f' % (ef, ms, S[:, 1].mean(), S[:, 0].mean(), passes.mean()))
    print('   max / mean of the per-query cycles: %.3f' % (tot.max() / tot.mean()))
    print('   total cycles per query: mean %.0f p50 %.0f p90 %.0f p99 %.0f max %.0f min %.0f ; implied clock if the max wave spans the kernel: %.2f GHz' % (
        tot.mean(), np.percentile(tot, 50), np.percentile(tot, 90), np.percentile(tot, 99), tot.max(), tot.min(), tot.max() / (ms * 1e6)))
    for i in (7, 0, 1, 2, 3, 8, 9, 5, 10, 4):
        print('   %-45s %9.0f cycles/query %5.1f%%   per pass %7.0f' % (names[i], D[:, i].mean(), 100 * D[:, i].mean() / tot.mean(), D[:, i].mean() / passes.mean()))
    print('   of slot 7: staging + entry point %.0f cycles/query (the entry point\'s distance is waited for at its end), the walk %.0f' % (
        D[:, 25].mean(), (D[:, 7] - D[:, 25]).mean()))
    # the front's own split (slots 40 .. 48; its stamps lengthen slot 7): staging alone, the per-layer clear, and per
    # upper-layer expansion the wait for the row it expands, the filter (look, claims), what is left of the row round
    # trip once the filter is done, and the chain; the rest of the walk is the winner, the next row's request, the branches
    if FRONT:
        nx = max(1.0, D[:, 48].mean())
        walk = (D[:, 7] - D[:, 25]).mean()
        parts = D[:, 41].mean() + D[:, 42].mean() + D[:, 43].mean() + D[:, 44].mean() + D[:, 45].mean()
        print('   front: staging %.0f, entry point %.0f, per-layer clear %.0f cycles/query; %.1f upper expansions, per expansion: wait for the row %.0f, look + claims %.0f, row round trip left %.0f, chain %.0f, winner + next request + rest %.0f; layer-0 table set-up %.0f cycles/query' % (
            D[:, 40].mean(), (D[:, 25] - D[:, 40]).mean(), D[:, 41].mean(), D[:, 48].mean(), D[:, 42].mean() / nx, D[:, 43].mean() / nx,
            D[:, 44].mean() / nx, D[:, 45].mean() / nx, (walk - parts) / nx, D[:, 47].mean()))
    acc = D[:, [0, 1, 2, 3, 5, 7, 8, 9, 10]].sum(1).mean()
    print('   unaccounted %.1f%%' % (100 * (tot.mean() - acc) / tot.mean()))
    print('   per query: visited slow-loop rounds %.1f; merges with 0 / 1-2 / >=3 survivors: %.1f / %.1f / %.1f; p commits %.1f' % (
        D[:, 11].mean(), D[:, 12].mean(), D[:, 13].mean(), D[:, 14].mean(), D[:, 15].mean()))
    # the merges' own split (slots 26 .. 30 c's merge, 31 .. 35 p's): cycles of the survivor loop, of the LDS phase and of
    # the shift path, the survivors of the big merges, the big merges.  (The split's own stamps lengthen slots 8 and 10.)
    for nm, b in (('merge c', 26), ('merge p', 31)):
        nbig, nsv = D[:, b + 4].sum(), D[:, b + 3].sum()
        print('   %s: survivor loop %.0f, LDS phase %.0f, shift path %.0f cycles/query; %.1f big merges of %.1f survivors: loop %.0f + LDS phase %.0f cycles per big merge, loop %.1f per survivor' % (
            nm, D[:, b].mean(), D[:, b + 1].mean(), D[:, b + 2].mean(), D[:, b + 4].mean(), nsv / max(1, nbig),
            D[:, b].sum() / max(1, nbig), D[:, b + 1].sum() / max(1, nbig), D[:, b].sum() / max(1, nsv)))
    # the small merges (slots 36 / 37 c's, 38 / 39 p's: merges that took the shift path, the keys they inserted); a small
    # merge holds one or two keys while HX_MERGE_SHIFT_MAX is 2: two-key merges = keys - merges
    for nm, b, c in (('merge c', 28, 36), ('merge p', 33, 38)):
        ns, nk = D[:, c].sum(), D[:, c + 1].sum()
        print('   %s: %.1f small merges of %.2f keys per query (with one key %.1f, with more %.1f): shift path %.0f cycles per small merge, %.0f per inserted key' % (
            nm, D[:, c].mean(), nk / max(1, ns), (2 * D[:, c] - D[:, c + 1]).clip(0).mean(), (D[:, c + 1] - D[:, c]).clip(None, D[:, c]).mean(),
            D[:, b].sum() / max(1, ns), D[:, b].sum() / max(1, nk)))
    # ... and what a merge costs by itself and what every key adds: least squares over the queries
    A = np.stack([D[:, 36] + D[:, 38], D[:, 37] + D[:, 39]], axis=1)
    fx, fk = np.linalg.lstsq(A, D[:, 28] + D[:, 33], rcond=None)[0]
    print('   shift path over the queries, least squares: %.0f cycles per small merge + %.0f per inserted key' % (fx, fk))
    # the runner-up's misses: c's merge puts a fresh key below p (slots 16 .. 22)
    miss = D[:, 16:19].sum(1)
    took = D[:, 22]
    print('   per query: misses %.1f, with 1 / 2 / >=3 fresh keys of c below p: %.1f / %.1f / %.1f; follow-up pick is the predicted pair %.2f; follow-up runner-up is the old p %.1f' % (
        miss.mean(), D[:, 16].mean(), D[:, 17].mean(), D[:, 18].mean(), D[:, 19].mean(), D[:, 20].mean()))
    # the frontier (the last three values: its cycles -- inside slot 0, which its own stamp lengthens --, its runs, and the
    # runs after c's merge: a survivor went in front of b, so the pair requested ahead is not the frontier's a and b)
    fr = D[:, SLOTS - 3:]
    print('   frontier: %.2f runs per pass, %.0f cycles per run at the pick; %.1f p commits per query, %.1f of them (%.1f%%) took the pair from the pick\'s frontier, %.1f ran it again' % (
        fr[:, 1].sum() / max(1, passes.sum()), fr[:, 0].sum() / max(1, (fr[:, 1] - fr[:, 2]).sum()), D[:, 15].mean(),
        (D[:, 15] - fr[:, 2]).mean(), 100 * (D[:, 15] - fr[:, 2]).sum() / max(1, D[:, 15].sum()), fr[:, 2].mean()))
    print('   pick + adjacency (slot 0) per pass: %.0f cycles on the %.1f passes whose rows were fetched ahead, %.0f on the %.1f others' % (
        D[:, 21].sum() / max(1, took.sum()), took.mean(), (D[:, 0] - D[:, 21]).sum() / max(1, (passes - took).sum()), (passes - took).mean()))
    print('   look + request + claims + chain (slot 1) per pass: %.0f cycles on the %.1f passes whose runner-up kept its distances, %.0f on the %.1f others' % (
        D[:, 23].sum() / max(1, D[:, 24].sum()), D[:, 24].mean(), (D[:, 1] - D[:, 23]).sum() / max(1, (passes - D[:, 24]).sum()), (passes - D[:, 24]).mean()))
    # what do the slowest queries look like?  (the kernel lasts as long as its slowest wave)
    order = np.argsort(-tot)[:8]
    print('   slowest queries: total cycles, n_exp, n_dist, passes, cycles/pass, slow-loop rounds, merges 0/1-2/>=3, p commits')
    for qi in order:
        print('     q%-5d %8.0f  n_exp %4d n_dist %5d passes %4d  %6.0f/pass  slow %3d  merges %3d/%3d/%3d  pcommits %3d' % (
            qi, tot[qi], S[qi, 1], S[qi, 0], passes[qi], tot[qi] / max(1, passes[qi]), D[qi, 11], D[qi, 12], D[qi, 13], D[qi, 14], D[qi, 15]))
        print('            misses 1/2/>=3 below p %3d/%3d/%3d  predicted %3d  old p again %3d  slot 0 per pass: ahead %5.0f (%3d passes), others %5.0f  slot 1 per pass %5.0f  kept %3d passes at %5.0f' % (
            D[qi, 16], D[qi, 17], D[qi, 18], D[qi, 19], D[qi, 20], D[qi, 21] / max(1, took[qi]), took[qi],
            (D[qi, 0] - D[qi, 21]) / max(1, passes[qi] - took[qi]), D[qi, 1] / max(1, passes[qi]), D[qi, 24], D[qi, 23] / max(1, D[qi, 24])))
        print('            merge c + p: survivor loop %6.0f  LDS phase %6.0f  shift path %6.0f cycles; big merges %3d with %4d survivors' % (
            D[qi, 26] + D[qi, 31], D[qi, 27] + D[qi, 32], D[qi, 28] + D[qi, 33], D[qi, 30] + D[qi, 35], D[qi, 29] + D[qi, 34]))
        print('            small merges %3d with %3d keys: shift path %5.0f cycles per small merge, %5.0f per key, %.1f%% of the query' % (
            D[qi, 36] + D[qi, 38], D[qi, 37] + D[qi, 39], (D[qi, 28] + D[qi, 33]) / max(1, D[qi, 36] + D[qi, 38]),
            (D[qi, 28] + D[qi, 33]) / max(1, D[qi, 37] + D[qi, 39]), 100 * (D[qi, 28] + D[qi, 33]) / tot[qi]))
    cc = np.corrcoef(tot, S[:, 1])[0, 1]
    fit = np.polyfit(S[:, 1].astype(np.float64), tot, 1)
    print('   corr(total cycles, n_exp) = %.3f; fit: cycles = %.0f * n_exp + %.0f; n_exp mean %.1f p99 %.0f max %d' % (
        cc, fit[0], fit[1], S[:, 1].mean(), np.percentile(S[:, 1], 99), S[:, 1].max()))
    res = tot - np.polyval(fit, S[:, 1].astype(np.float64))
    print('   residual of that fit: std %.0f, max %.0f, min %.0f' % (res.std(), res.max(), res.min()))
