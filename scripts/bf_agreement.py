"""Brute-force yardstick of the ANN engines at the bench's operating points.

On the bench library (2.1 M synthetic spectra of charge 2, seed 20240807, open window +-500 Da) the
brute-force open search (Config mode='bf': every library row of the precursor window is rescored)
and the ANN engines -- IVF-PQ m = 32 / nlist 4096 / nprobe 128 / k 1024 and IVF-Flat nprobe 112 --
answer the same 16 384 queries of synthetic.make_queries, default and hard. Reported per engine and
query set:
  * best_row_agreement: fraction of queries whose ANN best row is the brute-force best row (the
    reference notebook's measure);
  * bf_winner_in_topk: fraction whose brute-force winner is among the ANN top-k ids;
  * score gap brute force - ANN (mean, 99th percentile, fraction of queries with a gap);
and the brute-force time per batch and pairs scored per second. With `--ranks N` (2 .. 16) also
  * bf_winner_in_top_ranks: fraction whose brute-force winner is among the ANN path's N best
    rescored matches (the top-n rescoring, SpectralLibrary.search_batch_topn).

  python scripts/bf_agreement.py --out profiles/bf_agreement.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed_search(sl, q, mode, want_knn=False):
    torch.cuda.synchronize()
    t = time.perf_counter()
    res = sl._search_batch(q, 2, mode, want_knn=want_knn)   # host outputs: returns synchronised
    return res, time.perf_counter() - t


def agreement(res, b):
    """An engine's batch `res` (with its neighbour rows, if it has any) against the brute-force batch `b`."""
    has = b.best_row >= 0
    gap = np.where(has, b.best_score - np.where(res.best_row >= 0, res.best_score, 0.0), 0.0)
    out = {'best_row_agreement': float((res.best_row == b.best_row)[has].mean())}
    if res.knn is not None:
        in_topk = (res.knn == b.best_row[:, None].astype(np.int64)).any(1)
        out['bf_winner_in_topk'] = float(in_topk[has].mean())
    out.update(score_gap_mean=float(gap[has].mean()), score_gap_p99=float(np.percentile(gap[has], 99)),
               fraction_with_score_gap=float((gap[has] > 0).mean()),
               ann_score_above_bf=int((gap < 0).sum()))     # must be 0: the ANN lists are inside the window
    return out


def main():
    from ann_solo_amd import synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--library-size', type=int, default=2_100_000)
    ap.add_argument('--queries', type=int, default=16384)
    ap.add_argument('--open-da', type=float, default=500.0)
    ap.add_argument('--ranks', type=int, default=0,
                    help='also report whether the brute-force winner is among the N best rescored ANN matches')
    ap.add_argument('--out', default='bf_agreement.json')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    lib, aux = synthetic.make_library(args.library_size, seed=20240807, device=dev, charges=(2,), charge_p=(1.0,))
    qsets = {}
    for name, hard in (('default', 0.0), ('hard', synthetic.HARD_DEFAULT)):
        qsets[name], _ = synthetic.make_queries(lib, aux, args.queries, seed=42, open_range=args.open_da,
                                                charge=2, hard=hard)
    common = dict(precursor_tolerance_mass_open=args.open_da, precursor_tolerance_mode_open='Da',
                  batch_size=args.queries, seed=1234)
    out = {'library_size': lib.n, 'queries': args.queries, 'open_window_da': args.open_da,
           'hard_level': synthetic.HARD_DEFAULT, 'brute_force': {}, 'engines': {}}

    bf = SpectralLibrary(lib, config=Config.open_search(mode='bf', **common), device=dev)
    bf._search_batch(qsets['default'].select(torch.arange(256, device=dev)), 2, 'open')    # warm-up
    truth = {}
    for name, q in qsets.items():
        res, dt = timed_search(bf, q, 'open')
        pairs = int(res.n_candidates.astype(np.int64).sum())
        truth[name] = res
        out['brute_force'][name] = {'seconds_per_batch': dt, 'pairs': pairs, 'pairs_per_second': pairs / dt,
                                    'max_window': int(res.n_candidates.max()),
                                    'mean_window': float(res.n_candidates.mean())}
        print(f'[bf] {name}: {dt:.3f} s, {pairs} pairs, {pairs / dt / 1e9:.2f} G pairs/s', flush=True)
    bf.shutdown()

    engines = (('ivfpq_m32_nprobe128_k1024', dict(index='ivfpq', pq_m=32, num_probe=128)),
               ('ivfflat_nprobe112_k1024', dict(index='ivfflat', num_probe=112)))
    for ename, kw in engines:
        t = time.perf_counter()
        sl = SpectralLibrary(lib, config=Config.open_search(mode='ann', num_list=4096, num_candidates=1024,
                                                            kmeans_niter=25, **kw, **common), device=dev)
        sl._get_ann_index(2)
        build = time.perf_counter() - t
        out['engines'][ename] = {'index_build_seconds': build}
        for name, q in qsets.items():
            res, dt = timed_search(sl, q, 'open', want_knn=True)
            b = truth[name]
            has = b.best_row >= 0
            out['engines'][ename][name] = dict(agreement(res, b), ann_seconds_per_batch_unpipelined=dt)
            if args.ranks > 1:
                top = sl.search_batch_topn(q, 2, 'open', args.ranks)
                among = (top.best_row == b.best_row[:, None]).any(1)
                out['engines'][ename][name].update(ranks=args.ranks, bf_winner_in_top_ranks=float(among[has].mean()))
            print(f'[{ename}] {name}: {out["engines"][ename][name]}', flush=True)
        sl.shutdown()
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
