"""What a subset search costs: the selected scans against the plain ones, on the same build.

The bench library (2.1 M synthetic spectra of charge 2, seed 20240807; open window +-500 Da; batches of
32 768 queries, pipelined, device-resident inputs and outputs) at two operating points: configs[2]
(IVF-PQ m = 32, nlist 4096, nprobe 128, k 1024) and the fixed-recall point (IVF-Flat, nprobe 112).
Per index: the plain call, then `set_search_subset` with every row selected -- the price of the mechanism:
the selector words and the predicate -- then a random 50 %, 10 % and 1 % of the rows. The
configurations alternate, each run is warmed up and timed over `--steps` pipelined steps, `--rounds`
times. A second pass with the stage timers on reports scan / rescore / rescore_matches per batch, the
mean n_candidates, and how often the best match is the one a brute-force search (`use_ann = 0`) of the
same subset finds, over `--bf-queries` queries.

  python scripts/selector_cost.py --out profiles/selector_cost.json
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

SHARES = (1.0, 0.5, 0.1, 0.01)
POINTS = {'ivfpq': dict(index='ivfpq', pq_m=32, num_probe=128), 'ivfflat': dict(index='ivfflat', num_probe=112),
          # not in the default set: nprobe > 512 runs the two-probes-per-thread (WIDE) instantiations
          'ivfflat_wide': dict(index='ivfflat', num_probe=640), 'ivfpq_wide': dict(index='ivfpq', pq_m=32, num_probe=640)}
DEFAULT_POINTS = ('ivfpq', 'ivfflat')


def main():
    from ann_solo_amd import _lib, synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--library-size', type=int, default=2_100_000)
    ap.add_argument('--num-list', type=int, default=4096)
    ap.add_argument('--batch', type=int, default=32768)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kmeans-niter', type=int, default=25)
    ap.add_argument('--open-da', type=float, default=500.0)
    ap.add_argument('--bf-queries', type=int, default=2048)
    ap.add_argument('--indexes', nargs='+', default=list(DEFAULT_POINTS), choices=list(POINTS))
    ap.add_argument('--out', default='selector_cost.json')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    L = _lib.lib()
    lib, aux = synthetic.make_library(args.library_size, seed=20240807, device=dev, charges=(2,), charge_p=(1.0,))
    batches = [synthetic.make_queries(lib, aux, args.batch, seed=42 + i, open_range=args.open_da, charge=2)[0]
               .to(dev).contiguous() for i in range(2)]
    bfq = batches[0].select(torch.arange(min(args.bf_queries, args.batch), device=dev)).contiguous()
    rng = np.random.default_rng(7)
    draw = rng.random(lib.n)
    subsets = {'plain': None}
    subsets.update({'selected_%g' % s: torch.as_tensor(draw < s, device=dev) for s in SHARES})
    out = {'library_size': lib.n, 'batch': args.batch, 'steps': args.steps, 'warmup': args.warmup,
           'num_list': args.num_list, 'open_window_da': args.open_da, 'library': os.path.basename(_lib.LIB_PATH),
           'points': {}}
    for name in args.indexes:
        sl = SpectralLibrary(lib, config=Config.open_search(
            mode='ann', num_list=args.num_list, num_candidates=1024, kmeans_niter=args.kmeans_niter,
            precursor_tolerance_mass_open=args.open_da, precursor_tolerance_mode_open='Da', batch_size=args.batch,
            seed=1234, **POINTS[name]), device=dev)
        sl._get_ann_index(2)
        res = {'ms_per_step': {k: [] for k in subsets}, 'stages': {}}

        def step(i):
            return sl._search_batch(batches[i % 2], 2, 'open', device_out=True)

        def timed():
            sl.set_pipeline(True)
            try:
                for i in range(args.warmup):
                    step(i)
                sl.synchronize()
                t = time.perf_counter()
                for i in range(args.steps):
                    step(i)
                sl.synchronize()
                return (time.perf_counter() - t) / args.steps * 1e3
            finally:
                sl.set_pipeline(False)
        for _ in range(args.rounds):
            for k, keep in subsets.items():
                sl.set_search_subset(None if keep is None else {2: keep})
                res['ms_per_step'][k].append(round(timed(), 4))
                print(f'[step] {name} {k}: {res["ms_per_step"][k][-1]:.3f} ms', flush=True)
        for k, keep in subsets.items():      # second pass: the stage timers, candidates, brute-force agreement
            sl.set_search_subset(None if keep is None else {2: keep})
            L.asl_profile_reset()
            L.asl_profile_enable(1)
            for i in range(6):
                r = step(i)
            torch.cuda.synchronize()
            L.asl_profile_enable(0)
            st = {}
            for stage in ('scan', 'rescore', 'rescore_matches'):
                ms, n = C.c_double(), C.c_int64()
                L.asl_profile_get(stage.encode(), C.byref(ms), C.byref(n))
                st[stage] = round(ms.value / max(n.value, 1), 4)
            st['mean_n_candidates'] = round(float(r.n_candidates.float().mean().item()), 2)
            ann = sl._search_batch(bfq, 2, 'open', device_out=True)
            cfg_mode, sl.config.mode = sl.config.mode, 'bf'
            try:
                bf = sl._search_batch(bfq, 2, 'open', device_out=True)
            finally:
                sl.config.mode = cfg_mode
            torch.cuda.synchronize()
            st['bf_agreement'] = round(float((ann.best_row == bf.best_row).float().mean().item()), 4)
            res['stages'][k] = st
            print(f'[stages] {name} {k}: {st}', flush=True)
        sl.set_search_subset(None)
        sl.shutdown()
        out['points'][name] = res
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
