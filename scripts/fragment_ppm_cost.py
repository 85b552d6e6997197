"""What the ppm fragment tolerance costs the rescoring stage: the bench set-up (2.1 M synthetic spectra of
charge 2, seed 20240807, IVF-PQ m 32, nlist 4096, nprobe 128, k 1024, +-500 Da, 32 768 queries per batch), one
engine, synchronous batches, the device time of the `rescore` and `rescore_matches` stages (asl_profile_get)
at 0.02 Da and at 10 ppm, alternating. In ppm mode the bin filter keeps linear bins of the query's widest
window, so low-mass peaks share bins with more non-matching positions: the stage time says what that costs.
Also recorded: the candidates the flat kernel handed to the pair kernel (a doubly matched peak or a wide
exponent span), how many of them the winner-only pruning dropped, and the identifications that changed.

  python scripts/fragment_ppm_cost.py --out profiles/fragment_ppm_cost.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from ann_solo_amd import _lib, synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--library-size', type=int, default=2_100_000)
    ap.add_argument('--batch', type=int, default=32768)
    ap.add_argument('--nlist', type=int, default=4096)
    ap.add_argument('--niter', type=int, default=25)
    ap.add_argument('--da', type=float, default=0.02)
    ap.add_argument('--ppm', type=float, default=10.0)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default='fragment_ppm_cost.json')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    lib, aux = synthetic.make_library(args.library_size, seed=20240807, device=dev, charges=(2,), charge_p=(1.0,))
    q = synthetic.make_queries(lib, aux, args.batch, seed=42, open_range=500.0, charge=2)[0].to(dev).contiguous()
    cfg = Config.open_search(num_list=args.nlist, num_probe=128, num_candidates=1024, index='ivfpq', pq_m=32,
                             kmeans_niter=args.niter, mode='ann', precursor_tolerance_mass_open=500.0,
                             precursor_tolerance_mode_open='Da', batch_size=args.batch, seed=1234)
    sl = SpectralLibrary(lib, config=cfg, device=dev)
    L = _lib.lib()
    settings = (('Da', args.da), ('ppm', args.ppm))
    out = {'library_size': lib.n, 'batch': args.batch, 'steps': args.steps, 'runs': []}
    rows = {}
    for rnd in range(args.rounds + 1):             # round 0 warms up (index build, buffers)
        for unit, tol in settings:
            sl.config.fragment_tolerance_unit, sl.config.fragment_mz_tolerance = unit, tol
            L.asl_profile_reset()
            L.asl_profile_enable(1)
            for _ in range(args.steps if rnd else 1):
                r = sl._search_batch(q, 2, 'open', device_out=True)
            torch.cuda.synchronize()
            L.asl_profile_enable(0)
            if not rnd:
                continue
            run = {'unit': unit, 'tolerance': tol, 'round': rnd}
            for name in ('rescore', 'rescore_matches', 'scan'):
                ms, n = C.c_double(), C.c_int64()
                L.asl_profile_get(name.encode(), C.byref(ms), C.byref(n))
                run[name + '_ms_per_step'] = round(ms.value / args.steps, 4)
            d, p, w = C.c_int64(), C.c_int64(), C.c_int64()
            if hasattr(L, 'asl_profile_rescore_counts'):
                L.asl_profile_rescore_counts(C.byref(d), C.byref(p), C.byref(w))
                run.update(deferred_per_step=d.value // args.steps, pruned_per_step=p.value // args.steps)
            run['candidates_per_step'] = int(r.n_candidates.long().sum().item())
            run['mean_matched_peaks'] = round(float(r.pm_count.float().mean().item()), 3)
            rows[unit] = r.best_row.clone()
            out['runs'].append(run)
            print('[ppm-cost]', json.dumps(run), flush=True)
    out['winners_that_differ'] = int((rows['Da'] != rows['ppm']).sum().item())
    for unit, _ in settings:
        v = [r['rescore_ms_per_step'] for r in out['runs'] if r['unit'] == unit]
        out[f'rescore_ms_{unit}'] = {'min': min(v), 'max': max(v), 'mean': round(sum(v) / len(v), 4)}
    sl.shutdown()
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
