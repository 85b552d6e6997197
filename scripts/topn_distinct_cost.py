"""What the distinct ranked matches cost against the plain ones, on the same build.

The set-up of scripts/topn_cost.py (the bench library: 2.1 M synthetic spectra of charge 2, seed
20240807; IVF-PQ m = 32, nlist 4096, nprobe 128, k 1024; open window +-500 Da; batches of 32 768
queries, pipeline off, device-resident inputs and outputs). asl_search_batch_topn is timed against
asl_search_batch_topn_distinct at N = 1, 5, 16 with the library rows grouped 1, 3 and 20 to a group
(row // size); the configurations alternate, each run is warmed up and timed over `--steps`
device-synchronised steps, `--rounds` times. A second pass with the stage timers on reports the
`rescore` stage (scoring + selection: the selection kernel is the only launch that differs) and
`rescore_matches` per batch.

`--plain-only` times the plain calls alone: with ASL_LIB_PATH naming another build of the library
(the parent commit's) that is one side of a same-box A/B of the plain calls.

  python scripts/topn_distinct_cost.py --out profiles/topn_distinct_cost.json
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

RANKS = (1, 5, 16)
GROUP_SIZES = (1, 3, 20)


def timed(fn, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i in range(steps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def main():
    from ann_solo_amd import _lib, synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--library-size', type=int, default=2_100_000)
    ap.add_argument('--batch', type=int, default=32768)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--open-da', type=float, default=500.0)
    ap.add_argument('--plain-only', action='store_true')
    ap.add_argument('--ranks', type=int, nargs='+', default=list(RANKS))
    ap.add_argument('--group-sizes', type=int, nargs='+', default=list(GROUP_SIZES))
    ap.add_argument('--out', default='topn_distinct_cost.json')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    L = _lib.lib()
    lib, aux = synthetic.make_library(args.library_size, seed=20240807, device=dev, charges=(2,), charge_p=(1.0,))
    batches = [synthetic.make_queries(lib, aux, args.batch, seed=42 + i, open_range=args.open_da, charge=2)[0]
               .to(dev).contiguous() for i in range(2)]
    sl = SpectralLibrary(lib, config=Config.open_search(
        mode='ann', index='ivfpq', pq_m=32, num_list=4096, num_probe=128, num_candidates=1024, kmeans_niter=25,
        precursor_tolerance_mass_open=args.open_da, precursor_tolerance_mode_open='Da', batch_size=args.batch,
        seed=1234), device=dev)
    sl._get_ann_index(2)
    sl.set_pipeline(False)
    stride = max(b.max_peaks() for b in batches)
    n_lib = len(sl.partitions[2].ids)
    groups = {g: torch.as_tensor((np.arange(n_lib) // g).astype(np.int32), device=dev) for g in args.group_sizes}

    def plain(n):
        return lambda i: sl.search_batch_topn(batches[i % 2], 2, 'open', n, device_out=True, pm_stride=stride)

    def distinct(n):
        return lambda i: sl.search_batch_topn(batches[i % 2], 2, 'open', n, device_out=True, pm_stride=stride,
                                              distinct=True)
    out = {'library_size': lib.n, 'batch': args.batch, 'steps': args.steps, 'warmup': args.warmup,
           'index': 'ivfpq m32 nlist4096 nprobe128 k1024', 'open_window_da': args.open_da,
           'library': os.path.basename(_lib.LIB_PATH), 'ms_per_batch': {}, 'stage_ms_per_batch': {}}
    # (name, rows per group or None for the plain call, the call)
    runs = [('plain_%d' % n, None, plain(n)) for n in args.ranks]
    if not args.plain_only:
        runs += [('distinct_%d_group%d' % (n, g), g, distinct(n)) for g in args.group_sizes for n in args.ranks]

    def prepare(g):
        if g is not None:
            sl.set_match_groups({2: groups[g]})
    for name, _, _ in runs:
        out['ms_per_batch'][name] = []
    for _ in range(args.rounds):
        for name, g, fn in runs:
            prepare(g)
            for i in range(args.warmup):
                fn(i)
            out['ms_per_batch'][name].append(round(timed(fn, args.steps), 4))
            print(f'[batch] {name}: {out["ms_per_batch"][name][-1]:.3f} ms', flush=True)
    for name, g, fn in runs:            # second pass: the stage timers (events around every stage)
        prepare(g)
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
        out['stage_ms_per_batch'][name] = st
        print(f'[stages] {name}: {st}', flush=True)
    if not args.plain_only and 5 in args.ranks:
        # ranks filled and ranks that differ from the plain call's, per group size at N = 5
        base = plain(5)(0)
        out['ranks_at_5'] = {}
        for g in args.group_sizes:
            prepare(g)
            top = distinct(5)(0)
            torch.cuda.synchronize()
            out['ranks_at_5']['group%d' % g] = {
                'rank0_equal': bool(torch.equal(top.best_row[:, 0], base.best_row[:, 0])),
                'filled': int((top.best_row >= 0).sum().item()),
                'differ_from_plain': int((top.best_row != base.best_row).sum().item())}
    sl.shutdown()
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
