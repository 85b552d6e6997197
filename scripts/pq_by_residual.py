"""IVF-PQ on the raw hashed vectors (FAISS' by_residual = false) against the default residual codes, at
configs[2]: 2.1 M synthetic spectra of charge 2 (seed 20240807), nlist 4096, nprobe 128, k 1024, open
window +-500 Da, m = 32 x 8 bits. Both indexes are built in this process from the same vectors, with the
same seed (so the same coarse centroids and lists); the same with the exact re-rank (refine_k) on top.
Per mode, on default and hard queries of synthetic.make_queries:
  * recall@k against exact inner-product search, the same for IVF-Flat over the same lists and probes,
    and their ratio -- the fixed-recall criterion asks for >= 0.95 (bench.py: ratio_to_ivfflat) -- and
    the overlap with IVF-Flat's own rows;
  * hit@k of the generator's source row;
  * best-match agreement with the brute-force open search (scripts/bf_agreement.py's measure);
  * asl_index_rank: the share of brute-force winners / source rows with rank < 1, 10, 256, 1024 in the
    probed scope, without and with the precursor window (scripts/rank_curve.py's measure);
  * index training and add times (host clock around the synchronous calls); `--codec-only` stops after these
    and adds the add time of 262 144 random unit vectors at (800, 8, 8) -- codebooks of 102 400 B, staged in
    rounds -- with random unit quantisers installed by set_trained, and measures nothing else (the A/B of the
    quantiser kernels against another build of the library, ASL_LIB_PATH);
  * the pipelined step over `--steps` steps of `--batch` queries, `--rounds` alternating rounds, and the
    stage timers of ten more steps;
  * where in a query's probe order its top-k hits lie (mean probe position, share in the first 16 of the
    128 probes): with the coarse term in the score the early lists fill the top-k and the scan's
    threshold settles at once, without it hits keep arriving from every list.

  python scripts/pq_by_residual.py --out profiles/pq_by_residual.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (1, 10, 256, 1024)
MODES = (('by_residual', True), ('raw', False))


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def overlap(A, B):
    """mean over queries of |A_i & B_i| / k (rows of ids, -1 padded; on the device)"""
    k = A.shape[1]
    return sum(int(torch.isin(A[i][A[i] >= 0], B[i]).sum()) for i in range(A.shape[0])) / float(A.shape[0] * k)


def main():
    from ann_solo_amd import _lib, faiss_compat as faiss, synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--library-size', type=int, default=2_100_000)
    ap.add_argument('--nlist', type=int, default=4096)
    ap.add_argument('--nprobe', type=int, default=128)
    ap.add_argument('--k', type=int, default=1024)
    ap.add_argument('--niter', type=int, default=25)
    ap.add_argument('--batch', type=int, default=32768)
    ap.add_argument('--queries', type=int, default=2048, help='default and hard queries of the quality figures, each')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--refine-k', type=int, default=2048)
    ap.add_argument('--open-da', type=float, default=500.0)
    ap.add_argument('--out', default='pq_by_residual.json')
    ap.add_argument('--codec-only', action='store_true', help='train / add times only (see above)')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    lib, aux = synthetic.make_library(args.library_size, seed=20240807, device=dev, charges=(2,), charge_p=(1.0,))
    common = dict(precursor_tolerance_mass_open=args.open_da, precursor_tolerance_mode_open='Da',
                  batch_size=args.batch, seed=1234)
    ann = dict(mode='ann', index='ivfpq', pq_m=32, num_list=args.nlist, num_probe=args.nprobe,
               num_candidates=args.k, kmeans_niter=args.niter, **common)

    def build(by_res):
        """(engine, train seconds, add seconds) of one mode: the index is trained and filled here under the clock"""
        sl = SpectralLibrary(lib, config=Config.open_search(pq_by_residual=by_res, **ann), device=dev)
        vec = sl._encode(sl.partitions[2].spectra)
        ix = faiss.IndexIVFPQ(faiss.IndexFlatIP(vec.shape[1]), vec.shape[1], args.nlist, 32, 8)
        ix.by_residual = by_res
        ix.seed = 1234
        ix.set_niter(args.niter)
        _, t_train = clock(lambda: ix.train(vec))
        _, t_add = clock(lambda: ix.add(vec))
        return sl, ix, t_train, t_add

    def add_in_rounds(by_res, n=262144, d=800, m=8, nlist=256):
        """seconds of add() at (800, 8, 8): random unit vectors and quantisers, no training"""
        g = torch.Generator(device=dev).manual_seed(5)
        unit = lambda *shape: torch.nn.functional.normalize(torch.randn(*shape, generator=g, device=dev), dim=-1)
        ix = faiss.IndexIVFPQ(faiss.IndexFlatIP(d), d, nlist, m, 8)
        ix.by_residual = by_res
        ix.set_trained(unit(nlist, d).cpu().numpy(), unit(m, 256, d // m).cpu().numpy())
        x = unit(n, d).contiguous()
        ix.add(x[:4096])                  # warm-up: the code object is loaded
        return clock(lambda: ix.add(x))[1]

    if args.codec_only:
        fig = {}
        for mname, by_res in MODES:
            sl, ix, t_train, t_add = build(by_res)
            del ix
            sl.shutdown()
            fig[mname] = {'train_seconds': round(t_train, 4), 'add_seconds': round(t_add, 4),
                          'add_800_8_8_seconds': round(add_in_rounds(by_res), 4)}
        print(json.dumps({'library_size': lib.n, 'nlist': args.nlist, 'kmeans_niter': args.niter, 'lib': _lib.LIB_PATH,
                          'modes': fig}), flush=True)
        return
    nq = args.queries
    qsets, source = {}, {}
    for name, hard in (('default', 0.0), ('hard', synthetic.HARD_DEFAULT)):
        q, truth = synthetic.make_queries(lib, aux, nq, seed=42, open_range=args.open_da, charge=2, hard=hard)
        qsets[name], source[name] = q.to(dev).contiguous(), truth['source_row'][:nq].to(dev).to(torch.int64)
    batches = [synthetic.make_queries(lib, aux, args.batch, seed=42 + i, open_range=args.open_da, charge=2)[0]
               .to(dev).contiguous() for i in range(2)]
    out = {'library_size': lib.n, 'nlist': args.nlist, 'nprobe': args.nprobe, 'k': args.k, 'pq': 'm32 x 8 bits',
           'kmeans_niter': args.niter, 'open_window_da': args.open_da, 'queries': nq, 'batch': args.batch,
           'steps': args.steps, 'warmup': args.warmup, 'hard_level': synthetic.HARD_DEFAULT,
           'fixed_recall_criterion': 'recall@k vs exact IP >= 0.95 x IVF-Flat (same lists, same probes)',
           'modes': {}}

    # the brute-force winners (the yardstick of the agreement and of the rank curve)
    bf = SpectralLibrary(lib, config=Config.open_search(mode='bf', **common), device=dev)
    bf_best = {name: torch.as_tensor(bf._search_batch(q, 2, 'open').best_row, device=dev).to(torch.int64)
               for name, q in qsets.items()}
    bf.shutdown()
    print('[bf] done', flush=True)

    # the engine builds the same indexes again (same seed)
    sls = {}
    for mname, by_res in MODES:
        sl, ix, t_train, t_add = build(by_res)
        own = sl._get_ann_index(2)
        assert own.by_residual == by_res and np.array_equal(own.codebooks(), ix.codebooks())
        del ix
        sls[mname] = sl
        out['modes'][mname] = {'train_seconds': round(t_train, 3), 'add_seconds': round(t_add, 3)}
        print(f'[build] {mname}: train {t_train:.2f} s, add {t_add:.2f} s', flush=True)
    cen = sls['raw']._get_ann_index(2).centroids()
    assert np.array_equal(cen, sls['by_residual']._get_ann_index(2).centroids())      # same lists in both modes

    # exact inner products and IVF-Flat over the same lists and probes
    sl0 = sls['raw']
    vec = sl0._encode(sl0.partitions[2].spectra)
    xq = {name: sl0._encode(q) for name, q in qsets.items()}
    flat = faiss.IndexFlatIP(vec.shape[1])
    flat.add(vec)
    Ie = {name: flat.search(x, args.k)[1] for name, x in xq.items()}
    del flat
    fl = faiss.IndexIVFFlat(faiss.IndexFlatIP(vec.shape[1]), vec.shape[1], args.nlist)
    fl.set_trained(cen)
    fl.add(vec)
    fl.nprobe = args.nprobe
    If = {name: fl.search(x, args.k)[1] for name, x in xq.items()}
    del fl
    out['ivfflat'] = {name: {'recall_at_k_vs_exact_ip': overlap(If[name], Ie[name]),
                             'hit_at_k_source': float((If[name] == source[name].unsqueeze(1)).any(1).float().mean())}
                      for name in qsets}
    print('[ivfflat]', out['ivfflat'], flush=True)

    list_of = {}

    def probe_position(idx, x, knn):
        """probe position (0 = the best-scoring list) of the list of every hit of knn"""
        if 'v' not in list_of:          # the lists are the same in every index built here
            off, ids, _ = idx.lists()
            v = np.empty(lib.n, np.int64)
            v[ids] = np.repeat(np.arange(args.nlist), np.diff(off))
            list_of['v'] = torch.as_tensor(v, device=dev)
        _, cI = idx.coarse(x, args.nprobe)
        where = torch.full((x.shape[0], args.nlist), args.nprobe, dtype=torch.int64, device=dev)
        where.scatter_(1, cI.to(torch.int64), torch.arange(args.nprobe, device=dev).expand(x.shape[0], -1))
        ok = knn >= 0
        return where.gather(1, list_of['v'][knn.clamp_min(0)])[ok]

    def quality(sl, idx):
        res = {}
        key = torch.as_tensor(np.ascontiguousarray(sl.partitions[2].precursor_mz, np.float32), device=dev)
        for name, q in qsets.items():
            r = sl._search_batch(q, 2, 'open', want_knn=True, device_out=True)
            knn = r.knn
            rec, rf = overlap(knn, Ie[name]), out['ivfflat'][name]['recall_at_k_vs_exact_ip']
            best = r.best_row.to(torch.int64)
            pos = probe_position(idx, xq[name], knn)
            e = {'hit_probe_position_mean': float(pos.float().mean()),
                 'hits_in_first_16_probes': float((pos < 16).float().mean()),
                 'recall_at_k_vs_exact_ip': rec, 'ratio_to_ivfflat': rec / rf, 'meets_criterion': bool(rec / rf >= 0.95),
                 'overlap_with_ivfflat_rows': overlap(knn, If[name]),
                 'hit_at_k_source': float((knn == source[name].unsqueeze(1)).any(1).float().mean()),
                 'best_row_agreement_with_brute_force': float((best == bf_best[name]).float().mean()),
                 'bf_winner_in_topk': float(((knn == bf_best[name].unsqueeze(1)).any(1) | (bf_best[name] < 0))
                                            .float().mean())}
            if idx.refine_k == 0:       # the rank scan orders by the ADC score: the curve of the codes themselves
                e['rank_within_k'] = {}
                pmz = q.precursor_mz.to(torch.float64).contiguous()
                for tname, tgt in (('brute_force_winner', bf_best[name]), ('source_row', source[name])):
                    has = tgt >= 0
                    t = torch.where(has, tgt, torch.zeros_like(tgt)).contiguous()
                    for wname, win in (('no_window', None), ('window', (key, pmz, 2, args.open_da, 'Da'))):
                        rank = idx.rank_of(xq[name], t, nprobe=args.nprobe, window=win)[0][has]
                        n = max(int(has.sum()), 1)
                        e['rank_within_k'][f'{tname}/{wname}'] = {
                            str(k): float(((rank >= 0) & (rank < k)).sum()) / n for k in KS}
            res[name] = e
        return res

    for mname, _ in MODES:
        out['modes'][mname]['quality'] = quality(sls[mname], sls[mname]._get_ann_index(2))
        print(f'[quality] {mname}:', json.dumps(out['modes'][mname]['quality']), flush=True)

    # the pipelined step, alternating rounds
    times = {mname: [] for mname, _ in MODES}
    for _ in range(args.rounds):
        for mname, _ in MODES:
            sl = sls[mname]
            sl.set_pipeline(True)
            for i in range(args.warmup):
                sl._search_batch(batches[i % 2], 2, 'open', device_out=True)
            sl.synchronize()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for i in range(args.steps):
                sl._search_batch(batches[i % 2], 2, 'open', device_out=True)
            sl.synchronize()
            torch.cuda.synchronize()
            times[mname].append(round((time.perf_counter() - t) / args.steps * 1e3, 4))
            sl.set_pipeline(False)
            print(f'[step] {mname}: {times[mname][-1]:.3f} ms', flush=True)
    L = _lib.lib()
    for mname, _ in MODES:
        out['modes'][mname]['pipelined_ms_per_step'] = times[mname]
        sl = sls[mname]
        sl.set_pipeline(True)
        L.asl_profile_reset()
        L.asl_profile_enable(1)
        for i in range(10):
            sl._search_batch(batches[i % 2], 2, 'open', device_out=True)
        sl.synchronize()
        torch.cuda.synchronize()
        L.asl_profile_enable(0)
        sl.set_pipeline(False)
        st = {}
        for stage in ('coarse_gemm', 'coarse_select', 'scan', 'rescore', 'rescore_matches'):
            ms, n = C.c_double(), C.c_int64()
            L.asl_profile_get(stage.encode(), C.byref(ms), C.byref(n))
            st[stage] = round(ms.value / max(n.value, 1), 4)
        out['modes'][mname]['stage_ms_per_step'] = st
        print(f'[stages] {mname}: {st}', flush=True)
        sl.shutdown()
    del sls

    # the exact re-rank of the refine_k best ADC candidates on top of either code
    if args.refine_k > args.k:
        out['refine_k'] = args.refine_k
        for mname, by_res in MODES:
            sl = SpectralLibrary(lib, config=Config.open_search(pq_by_residual=by_res, refine_k=args.refine_k, **ann),
                                 device=dev)
            idx = sl._get_ann_index(2)
            assert idx.refine_k == args.refine_k and idx.by_residual == by_res
            out['modes'][mname]['quality_with_refine'] = quality(sl, idx)
            print(f'[refine] {mname}:', json.dumps(out['modes'][mname]['quality_with_refine']), flush=True)
            sl.shutdown()
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
