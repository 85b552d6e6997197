"""What an asymmetric open window saves a brute-force open search: one 16 384-query `--mode bf` batch on the
bench library (2.1 M synthetic spectra of charge 2, seed 20240807) at the symmetric +-500 Da window against
the signed range (-150, +500) Da given as per-query intervals (`windows=`, ASL_TOL_INTERVAL). Reports the
candidate pairs and the seconds of each batch, and the ratio of both: the expectation that the time follows
the pairs is checked here, not assumed.

  python scripts/interval_bf_cost.py --out profiles/interval_bf_cost.json
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from ann_solo_amd import synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary, open_window_intervals
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--library-size', type=int, default=2_100_000)
    ap.add_argument('--batch', type=int, default=16384)
    ap.add_argument('--open-da', type=float, default=500.0)
    ap.add_argument('--low', type=float, default=-150.0)
    ap.add_argument('--high', type=float, default=500.0)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--out', default='interval_bf_cost.json')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    lib, aux = synthetic.make_library(args.library_size, seed=20240807, device=dev, charges=(2,), charge_p=(1.0,))
    q = synthetic.make_queries(lib, aux, args.batch, seed=42, open_range=args.open_da, charge=2)[0].to(dev).contiguous()
    sl = SpectralLibrary(lib, config=Config.open_search(mode='bf', precursor_tolerance_mass_open=args.open_da,
                                                        precursor_tolerance_mode_open='Da', batch_size=args.batch),
                         device=dev)
    wins = torch.as_tensor(open_window_intervals(q.precursor_mz.cpu().numpy(), 2, (args.low, args.high)), device=dev)
    sl._search_batch(q.select(torch.arange(256, device=dev)).contiguous(), 2, 'open', device_out=True)   # warm-up
    torch.cuda.synchronize()
    out = {'library_size': lib.n, 'batch': args.batch, 'symmetric_da': args.open_da, 'range_da': [args.low, args.high],
           'runs': []}
    for _ in range(args.rounds):
        for name, w in (('symmetric', None), ('interval', wins)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = sl._search_batch(q, 2, 'open', device_out=True) if w is None else \
                sl._search_batch(q, 2, 'open', device_out=True, windows=w)
            torch.cuda.synchronize()
            sec = time.perf_counter() - t
            pairs = int(r.n_candidates.long().sum().item())
            out['runs'].append({'window': name, 'pairs': pairs, 'seconds': round(sec, 4),
                                'gpairs_per_s': round(pairs / sec / 1e9, 4)})
            print(f'[bf] {name}: {pairs} pairs in {sec:.3f} s', flush=True)
    sym = [r for r in out['runs'] if r['window'] == 'symmetric'][-1]
    itv = [r for r in out['runs'] if r['window'] == 'interval'][-1]
    out['pairs_ratio'] = round(itv['pairs'] / max(sym['pairs'], 1), 4)
    out['seconds_ratio'] = round(itv['seconds'] / sym['seconds'], 4)
    sl.shutdown()
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
