"""Window scan sweep: Config.ann_window = 'post' (the reference's order) against 'pre' (the k best
in-window vectors of the probed lists) at the bench's configs[2] point.

Library and queries of bench.py (2.1 M synthetic spectra of charge 2, seed 20240807; 32 768-query
batches of synthetic.make_queries, seed 42, open +-500 Da), IVF-PQ m 32 / nlist 4096, pipelined and warm.
Rows: post k 1024 nprobe 128; pre k 128 / 256 / 512 / 1024 nprobe 128; pre k 256 nprobe 256. Per row:
  * step_ms: pipelined steps (device outputs), after warm-up;
  * scan_ms / window_ranges_ms / rescore_ms: per step, a second pass with every stage bracketed;
  * mean_n_cand: candidates the rescoring scored per query;
  * scanned_vectors_per_query (the device count: sum of hi - lo for 'pre', whole probed lists for
    'post'), its bytes at 36 B per vector, and the 64-vector tiles touched per query (host count; for
    'pre' from the interval q +- tol / z, which may differ from the kernel's exact test at the edges);
  * agreement with brute-force open search (scripts/bf_agreement.py's yardstick) on 2 048 default and
    2 048 hard queries: best_row_agreement and bf_winner_in_topk;
  * layout_build_s ('pre'): the first batch's extra time, in which the window-ordered layout is built.

  python scripts/window_scan_sweep.py --out profiles/window_scan_sweep.json
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

ROWS = (('post', 1024, 128), ('pre', 128, 128), ('pre', 256, 128), ('pre', 512, 128), ('pre', 1024, 128),
        ('pre', 256, 256))


def tiles_touched(idx, xq, q_pmz, nprobe, key, half_width):
    """64-vector tiles per query the scan reads: whole probed lists ('post', half_width None) or the
    run of each probed list inside q +- half_width in the key-sorted order ('pre')."""
    off, ids, _ = idx.lists()
    _, I = idx.coarse(xq, nprobe)
    I = np.asarray(I.cpu().numpy() if hasattr(I, 'cpu') else I, np.int64)
    off = np.asarray(off, np.int64)
    lens = np.diff(off)
    if half_width is None:
        return float(((lens[I] + 63) // 64).sum() / len(xq)), float(lens[I].sum() / len(xq))
    lst = np.repeat(np.arange(len(lens)), lens)
    k = np.asarray(key, np.float64)[np.asarray(ids)]
    comb = np.sort(lst * 1e5 + np.nan_to_num(k, nan=9e4))     # per list ascending, NaN last
    base = I * 1e5
    lo = np.searchsorted(comb, base + (q_pmz[:, None] - half_width), 'left') - off[I]
    hi = np.searchsorted(comb, base + (q_pmz[:, None] + half_width), 'right') - off[I]
    t = np.where(hi > lo, ((hi - 1) >> 6) - (lo >> 6) + 1, 0)
    return float(t.sum() / len(xq)), float((hi - lo).sum() / len(xq))


def main():
    from ann_solo_amd import _lib, synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--library-size', type=int, default=2_100_000)
    ap.add_argument('--batch', type=int, default=32768)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--agreement-queries', type=int, default=2048)
    ap.add_argument('--open-da', type=float, default=500.0)
    ap.add_argument('--out', default='window_scan_sweep.json')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    L = _lib.lib()
    lib, aux = synthetic.make_library(args.library_size, seed=20240807, device=dev, charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, args.batch, seed=42, open_range=args.open_da, charge=2)
    qsets = {}
    for name, hard in (('default', 0.0), ('hard', synthetic.HARD_DEFAULT)):
        qsets[name], _ = synthetic.make_queries(lib, aux, args.agreement_queries, seed=42, open_range=args.open_da,
                                                charge=2, hard=hard)
    common = dict(precursor_tolerance_mass_open=args.open_da, precursor_tolerance_mode_open='Da',
                  batch_size=args.batch, seed=1234)
    out = {'library_size': lib.n, 'batch': args.batch, 'steps': args.steps, 'warmup': args.warmup,
           'open_window_da': args.open_da, 'nlist': 4096, 'pq_m': 32, 'agreement_queries': args.agreement_queries,
           'hard_level': synthetic.HARD_DEFAULT, 'rows': []}
    bf = SpectralLibrary(lib, config=Config.open_search(mode='bf', **common), device=dev)
    truth = {name: bf._search_batch(qq, 2, 'open') for name, qq in qsets.items()}
    bf.shutdown()
    print('[sweep] brute force done', flush=True)

    q_pmz = q.precursor_mz.double().cpu().numpy()
    for window, k, nprobe in ROWS:
        cfg = Config.open_search(mode='ann', index='ivfpq', pq_m=32, num_list=4096, num_probe=nprobe,
                                 num_candidates=k, kmeans_niter=25, ann_window=window, **common)
        sl = SpectralLibrary(lib, config=cfg, device=dev)
        idx = sl._get_ann_index(2)
        row = {'ann_window': window, 'k': k, 'nprobe': nprobe}
        small = q.select(torch.arange(256, device=dev)).contiguous()
        t0 = time.perf_counter()
        sl._search_batch(small, 2, 'open')
        t1 = time.perf_counter()
        sl._search_batch(small, 2, 'open')
        t2 = time.perf_counter()
        row['layout_build_s'] = round((t1 - t0) - (t2 - t1), 4) if window == 'pre' else 0.0
        res = sl._search_batch(q, 2, 'open')
        row['mean_n_cand'] = float(res.n_candidates.mean())
        sl.set_pipeline(True)
        for _ in range(args.warmup):
            sl._search_batch(q, 2, 'open', device_out=True)
        sl.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            r = sl._search_batch(q, 2, 'open', device_out=True)
        sl.synchronize()
        row['step_ms'] = round((time.perf_counter() - t0) / args.steps * 1e3, 3)
        assert np.array_equal(r.best_row.cpu().numpy(), res.best_row)     # pipelined == synchronous
        L.asl_profile_reset()
        L.asl_profile_enable(1)
        for _ in range(args.steps):
            sl._search_batch(q, 2, 'open', device_out=True)
        sl.synchronize()
        L.asl_profile_enable(0)
        sl.set_pipeline(False)
        for stage in ('scan', 'window_ranges', 'rescore', 'rescore_matches', 'encode', 'coarse_gemm', 'coarse_select'):
            ms, n = C.c_double(), C.c_int64()
            L.asl_profile_get(stage.encode(), C.byref(ms), C.byref(n))
            row[f'{stage}_ms'] = round(ms.value / args.steps, 3)
        scanned = L.asl_profile_scanned_vectors() / (args.steps * q.n)
        row['scanned_vectors_per_query'] = round(scanned, 1)
        row['scanned_bytes_per_query'] = round(36 * scanned, 1)
        xq = sl._encode(q)
        tiles, vecs = tiles_touched(idx, xq, q_pmz, nprobe, sl.partitions[2].precursor_mz,
                                    None if window == 'post' else args.open_da / 2)
        row['tiles_touched_per_query'] = round(tiles, 1)
        row['host_count_vectors_per_query'] = round(vecs, 1)
        for name, qq in qsets.items():
            a = sl._search_batch(qq, 2, 'open', want_knn=True)
            b = truth[name]
            has = b.best_row >= 0
            in_topk = (a.knn == b.best_row[:, None].astype(np.int64)).any(1)
            row[f'{name}_best_row_agreement'] = round(float((a.best_row == b.best_row)[has].mean()), 4)
            row[f'{name}_bf_winner_in_topk'] = round(float(in_topk[has].mean()), 4)
        sl.shutdown()
        out['rows'].append(row)
        print(f'[sweep] {row}', flush=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
