"""Rank of the correct neighbour in the index's neighbour order: the measurement the reference chooses
num_candidates and num_probe from (notebooks/iprg2012_num_candidates.ipynb: IndexFlatIP searched with
num_neighbors = 1000000, then the position of the brute-force match), made with asl_index_rank.

On the bench library (2.1 M synthetic spectra of charge 2, seed 20240807, nlist 4096, open window +-500 Da)
2 048 default and 2 048 hard queries of synthetic.make_queries are ranked against two targets -- the
brute-force best row (Config mode='bf', as scripts/bf_agreement.py) and the generator's source row -- in
IVF-Flat and IVF-PQ (m = 32), with and without the precursor window, over the exhaustive scope (nprobe 0)
and nprobe 128 / 256 / 1024. Per combination:
  * within_k: the share of targets identified with 1 / 10 / 256 / 1024 / 5000 neighbours (rank < k);
  * neighbours_for: the neighbours needed for 90 / 95 / 99 % of the targets (null: never reached);
  * not_in_scope: the share with rank = -1 (list not probed, or outside the window) against
    beyond_k[k]: the share with 0 <= rank but rank >= k -- "its list was not probed" apart from "k was too small";
  * seconds_per_call: host clock around the synchronous call (it ends in a stream synchronise), the
    median of `--repeats` calls after one warm-up call of the same shape.
Beside that the only other route to a (weaker) answer, IVF-Flat search at k = 16384, is timed on the
same queries in the same process.

  python scripts/rank_curve.py --out profiles/rank_curve.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (1, 10, 256, 1024, 5000)
SHARES = (0.90, 0.95, 0.99)


def timed(fn, repeats):
    fn()                                    # warm-up: code objects, buffers of this shape
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return out, float(np.median(ts)), ts


def curve(rank, has):
    """The notebook's figures over the queries that have a target."""
    r = rank[has]
    n = max(len(r), 1)
    inside = np.sort(r[r >= 0])
    need = {}
    for s in SHARES:
        j = int(np.ceil(s * n)) - 1         # the rank of the query that completes the share
        need[f'{int(s * 100)}%'] = int(inside[j]) + 1 if j < len(inside) else None
    return {'targets': int(len(r)),
            'within_k': {str(k): float(((r >= 0) & (r < k)).sum() / n) for k in KS},
            'neighbours_for': need,
            'not_in_scope': float((r < 0).sum() / n),
            'beyond_k': {str(k): float((r >= k).sum() / n) for k in KS},
            'median_rank': int(np.median(inside)) if len(inside) else None,
            'max_rank': int(inside[-1]) if len(inside) else None}


def main():
    from ann_solo_amd import synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--library-size', type=int, default=2_100_000)
    ap.add_argument('--queries', type=int, default=2048)
    ap.add_argument('--num-list', type=int, default=4096)
    ap.add_argument('--open-da', type=float, default=500.0)
    ap.add_argument('--scopes', type=int, nargs='+', default=[0, 128, 256, 1024])
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default='rank_curve.json')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('rank_curve.py measures on the GPU: no device found')
    dev = torch.device('cuda', 0)
    lib, aux = synthetic.make_library(args.library_size, seed=20240807, device=dev, charges=(2,), charge_p=(1.0,))
    qsets, source = {}, {}
    for name, hard in (('default', 0.0), ('hard', synthetic.HARD_DEFAULT)):
        qsets[name], truth = synthetic.make_queries(lib, aux, args.queries, seed=42, open_range=args.open_da,
                                                    charge=2, hard=hard)
        source[name] = truth['source_row'].cpu().numpy().astype(np.int64)
    common = dict(precursor_tolerance_mass_open=args.open_da, precursor_tolerance_mode_open='Da',
                  batch_size=args.queries, seed=1234)
    out = {'library_size': lib.n, 'queries': args.queries, 'num_list': args.num_list, 'open_window_da': args.open_da,
           'hard_level': synthetic.HARD_DEFAULT, 'ks': list(KS), 'repeats': args.repeats, 'engines': {}}

    bf = SpectralLibrary(lib, config=Config.open_search(mode='bf', **common), device=dev)
    best = {name: bf._search_batch(q, 2, 'open').best_row.astype(np.int64) for name, q in qsets.items()}
    bf.shutdown()
    targets = {'bf_best_row': best, 'source_row': source}

    for ename, kw in (('ivfflat', dict(index='ivfflat')), ('ivfpq_m32', dict(index='ivfpq', pq_m=32))):
        sl = SpectralLibrary(lib, config=Config.open_search(mode='ann', num_list=args.num_list, num_probe=128,
                                                            num_candidates=1024, kmeans_niter=25, **kw, **common),
                             device=dev)
        idx = sl._get_ann_index(2)
        eng = out['engines'][ename] = {}
        for qname, q in qsets.items():
            for tname, tg in targets.items():
                rows = tg[qname]
                has = rows >= 0
                for window in (False, True):
                    for nprobe in args.scopes:
                        scope_name = 'exhaustive' if nprobe == 0 else f'nprobe{nprobe}'
                        (rank, _, scope), dt, ts = timed(
                            lambda: sl.candidate_rank(q, 2, rows, nprobe=nprobe, window=window), args.repeats)
                        rec = curve(rank, has)
                        rec.update(seconds_per_call=dt, seconds_each=ts, mean_scope=float(scope.mean()))
                        eng.setdefault(qname, {}).setdefault(tname, {}).setdefault(
                            'window' if window else 'no_window', {})[scope_name] = rec
                        print(f'[{ename}] {qname} {tname} window={window} {scope_name}: {dt * 1e3:.1f} ms, '
                              f'within {rec["within_k"]}, not in scope {rec["not_in_scope"]:.4f}', flush=True)
        if ename == 'ivfflat':
            # the existing route to a weaker answer: the 16 384 best neighbours, then look the target up
            xq = {name: sl._encode(q.to(dev)) for name, q in qsets.items()}
            for nprobe in (n for n in args.scopes if n):
                idx.nprobe = nprobe
                for qname in qsets:
                    (_, I), dt, ts = timed(lambda: idx.search(xq[qname], 16384), 1)
                    found = (I == torch.as_tensor(best[qname], device=dev)[:, None]).any(1).cpu().numpy()
                    out.setdefault('ivfflat_search_k16384', {}).setdefault(qname, {})[f'nprobe{nprobe}'] = {
                        'seconds_per_call': dt, 'bf_best_row_within_16384': float(found[best[qname] >= 0].mean())}
                    print(f'[ivfflat search k=16384] {qname} nprobe{nprobe}: {dt:.3f} s', flush=True)
            idx.nprobe = 128
        sl.shutdown()
        with open(args.out, 'w') as f:      # after every engine: a later failure keeps what was measured
            json.dump(out, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
