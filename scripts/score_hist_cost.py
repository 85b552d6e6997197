"""What the score histogram costs at the bench's operating point.

On the bench library (2.1 M synthetic spectra of charge 2, seed 20240807; IVF-PQ m = 32, nlist 4096,
nprobe 128, k 1024; open window +-500 Da; batches of 32 768 queries, pipeline off, device-resident
inputs and outputs) the synchronous asl_search_batch_topn at N = 1 is timed against
asl_search_batch_topn_hist at N = 1: the two alternate, each run is warmed up and timed over `--steps`
device-synchronised steps, `--rounds` times. A second pass with the stage timers on (asl_profile_get)
reports the `rescore` stage (scoring + histogram + selection) per batch. Last, one brute-force batch
(use_ann = 0, `--bf-queries` queries, tiled by the pair budget) with and without the histogram. Every
histogram is checked: its rows sum to n_cand and the other outputs equal the plain call's.

  python scripts/score_hist_cost.py --out profiles/score_hist_cost.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i in range(steps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def same(a, b):
    return bool(torch.equal(a.best_row, b.best_row) and torch.equal(a.best_score, b.best_score) and
                torch.equal(a.n_candidates, b.n_candidates) and torch.equal(a.pm_count, b.pm_count) and
                torch.equal(a.pm_pairs, b.pm_pairs) and
                torch.equal(b.score_hist.sum(dim=1, dtype=torch.int64), b.n_candidates.to(torch.int64)))


def main():
    from ann_solo_amd import _lib, synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--library-size', type=int, default=2_100_000)
    ap.add_argument('--batch', type=int, default=32768)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--bf-queries', type=int, default=2048)
    ap.add_argument('--open-da', type=float, default=500.0)
    ap.add_argument('--out', default='score_hist_cost.json')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    L = _lib.lib()
    lib, aux = synthetic.make_library(args.library_size, seed=20240807, device=dev, charges=(2,), charge_p=(1.0,))
    batches = [synthetic.make_queries(lib, aux, args.batch, seed=42 + i, open_range=args.open_da, charge=2)[0]
               .to(dev).contiguous() for i in range(2)]
    common = dict(precursor_tolerance_mass_open=args.open_da, precursor_tolerance_mode_open='Da',
                  batch_size=args.batch, seed=1234)
    sl = SpectralLibrary(lib, config=Config.open_search(mode='ann', index='ivfpq', pq_m=32, num_list=4096,
                                                        num_probe=128, num_candidates=1024, kmeans_niter=25,
                                                        **common), device=dev)
    sl._get_ann_index(2)
    sl.set_pipeline(False)
    stride = max(b.max_peaks() for b in batches)
    calls = {'topn_1': lambda i: sl.search_batch_topn(batches[i % 2], 2, 'open', 1, device_out=True, pm_stride=stride),
             'topn_1_hist': lambda i: sl.search_batch_topn(batches[i % 2], 2, 'open', 1, device_out=True,
                                                           pm_stride=stride, score_hist=True)}
    out = {'library_size': lib.n, 'batch': args.batch, 'steps': args.steps, 'warmup': args.warmup,
           'index': 'ivfpq m32 nlist4096 nprobe128 k1024', 'open_window_da': args.open_da,
           'ann_ms_per_batch': {name: [] for name in calls}, 'ann_stage_ms_per_batch': {}, 'brute_force': {}}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            for i in range(args.warmup):
                fn(i)
            out['ann_ms_per_batch'][name].append(round(timed(fn, args.steps), 4))
            print(f'[ann] {name}: {out["ann_ms_per_batch"][name][-1]:.3f} ms', flush=True)
    a, b = calls['topn_1'](0), calls['topn_1_hist'](0)
    torch.cuda.synchronize()
    out['outputs_equal_and_rows_sum_to_n_cand'] = same(a, b)
    out['mean_candidates_per_query'] = round(float(b.n_candidates.double().mean().item()), 2)
    mean = {k: sum(v) / len(v) for k, v in out['ann_ms_per_batch'].items()}
    out['ann_hist_cost_ms_per_batch'] = round(mean['topn_1_hist'] - mean['topn_1'], 4)
    out['ann_hist_cost_percent'] = round(100.0 * (mean['topn_1_hist'] / mean['topn_1'] - 1.0), 3)
    for name, fn in calls.items():      # second pass: the stage timers (events around every stage)
        L.asl_profile_reset()
        L.asl_profile_enable(1)
        for i in range(10):
            fn(i)
        torch.cuda.synchronize()
        L.asl_profile_enable(0)
        st = {}
        for stage in ('scan', 'rescore', 'rescore_matches'):
            ms, n = C.c_double(), C.c_int64()
            L.asl_profile_get(stage.encode(), C.byref(ms), C.byref(n))
            st[stage] = round(ms.value / max(n.value, 1), 4)
        out['ann_stage_ms_per_batch'][name] = st
        print(f'[stages] {name}: {st}', flush=True)
    sl.shutdown()

    bf = SpectralLibrary(lib, config=Config.open_search(mode='bf', **common), device=dev)
    q = batches[0].select(torch.arange(args.bf_queries, device=dev)).contiguous()
    bf_calls = {'topn_1': lambda i: bf.search_batch_topn(q, 2, 'open', 1, device_out=True, pm_stride=stride),
                'topn_1_hist': lambda i: bf.search_batch_topn(q, 2, 'open', 1, device_out=True, pm_stride=stride,
                                                              score_hist=True)}
    bf_calls['topn_1'](0)               # warm-up: the scratch of a tile
    res = {name: [] for name in bf_calls}
    for _ in range(args.rounds):
        for name, fn in bf_calls.items():
            res[name].append(round(timed(fn, 1), 3))
            print(f'[bf] {name}: {res[name][-1]:.1f} ms', flush=True)
    a, b = bf_calls['topn_1'](0), bf_calls['topn_1_hist'](0)
    torch.cuda.synchronize()
    pairs = int(a.n_candidates.to(torch.int64).sum().item())
    out['brute_force'] = {'queries': args.bf_queries, 'pairs': pairs, 'ms_per_batch': res,
                          'outputs_equal_and_rows_sum_to_n_cand': same(a, b)}
    bf.shutdown()
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
