"""What the window-exact index (`Config.index = 'winflat'`) costs and what agreement it buys, beside the two ANN
operating points of the bench, from one build on one GPU.

Geometry: the bench's library (2.1 M synthetic spectra of charge 2, seed 20240807), k 1 024, open window +-500 Da,
32 768-query pipelined steps, three alternating rounds over the engines. Per engine: ms per step (mean and the
rounds), scan / run-search / rescoring ms per step from a second, stage-bracketed pass, the vectors scanned per
query (winflat: the sum of hi - lo of the runs). Agreement: on 2 048 default and 2 048 hard queries, the fraction
whose best match is the brute-force one (`Config.mode = 'bf'`, the measure of scripts/bf_agreement.py), for the
three points and for winflat at k 256, by `agreement` of scripts/bf_agreement.py.

Algorithmic work of the ranged scan, counted (`ranged_work`): the layout is rebuilt here from the library's key
column and the encoded vectors -- the same order (key ascending, id ascending), the same 832-position blocks --
as the number of postings per (block, dimension); a query's run [lo, hi) comes from the window test itself, and
over its blocks lo / 832 .. (hi - 1) / 832 and its non-zero dimensions the work is summed by the definitions of
flat_postings_work_kernel (csrc/flat_tools.hip): float postings, 4-byte table word + 6 bytes per posting; fixed-point
words, table byte + 4 bytes per posting (lines: the block's table row + the whole lines of the segments). The sum of
hi - lo is checked against
asl_profile_scanned_vectors. IVF-Flat's own figure comes from asl_index_postings_work over a sample of the batch.

  python scripts/winflat_cost.py --out profiles/winflat_cost.json
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


FI_BLK = 832


def ranged_work(sl, q, tol_da, charge, fx):
    """Per 32 768-query batch `q`: (vectors in the runs, blocks listed, algorithmic bytes, 128-byte lines or None)
    of the ranged postings scan over the window-exact layout of `sl`'s charge partition."""
    part, dev = sl.partitions[charge], sl.device
    key = torch.as_tensor(np.asarray(part.precursor_mz, np.float32), device=dev)
    order = torch.argsort(key, stable=True)                 # (no NaN keys in this library)
    skey = key[order].double()
    n, d = len(key), sl.config.hash_len
    nblk = (n + FI_BLK - 1) // FI_BLK
    cnt = torch.zeros((nblk, d), dtype=torch.int64, device=dev)
    step = 64
    for b0 in range(0, nblk, step):
        rows = order[b0 * FI_BLK:(b0 + step) * FI_BLK]
        x = sl._encode(part.spectra.select(rows))
        if fx:      # what add() stores in fixed-point mode (fx22_round)
            x = torch.where((x >= 0) & (x < 1), torch.round(x * 4194304.0).clamp(max=4194303.0) / 4194304.0, x)
        nz = (x != 0).to(torch.int64)
        pad = (-len(rows)) % FI_BLK
        if pad:
            nz = torch.cat([nz, torch.zeros((pad, d), dtype=torch.int64, device=dev)])
        cnt[b0:b0 + nz.shape[0] // FI_BLK] = nz.view(-1, FI_BLK, d).sum(1)
    zero = torch.zeros((1, d), dtype=torch.int64, device=dev)
    P_c = torch.cat([zero, cnt.cumsum(0)])
    P_l = torch.cat([zero, ((cnt + 31) // 32).cumsum(0)])
    qp = q.precursor_mz.double().to(dev)
    ok = lambda pos: (pos >= 0) & (pos < n) & ((qp - skey[pos.clamp(0, n - 1)]).abs() * float(charge) <= tol_da)
    lo = torch.searchsorted(skey, qp - tol_da / charge)
    hi = torch.searchsorted(skey, qp + tol_da / charge, right=True)
    for _ in range(4):      # the edges by the window test itself
        lo = torch.where(ok(lo - 1), lo - 1, torch.where(~ok(lo) & (lo < hi), lo + 1, lo))
        hi = torch.where(ok(hi), hi + 1, torch.where(~ok(hi - 1) & (hi > lo), hi - 1, hi))
    b_first, b_last = lo // FI_BLK, (hi - 1).clamp(min=0) // FI_BLK
    blocks = torch.where(hi > lo, b_last - b_first + 1, torch.zeros_like(lo))
    b_end = torch.where(hi > lo, b_last + 1, b_first)
    vectors = bytes_ = lines = 0
    for a in range(0, q.n, 4096):
        sel = torch.arange(a, min(a + 4096, q.n), device=dev)
        qmask = (sl._encode(q.select(sel)) != 0).to(torch.int64)
        K = qmask.sum(1)
        posts = ((P_c[b_end[sel]] - P_c[b_first[sel]]) * qmask).sum(1)
        vectors += int((hi - lo)[sel].sum())
        if fx:
            bytes_ += int((K * blocks[sel] + 4 * posts).sum())
            lines += int((((P_l[b_end[sel]] - P_l[b_first[sel]]) * qmask).sum(1) + blocks[sel] * ((d + 127) // 128)).sum())
        else:
            bytes_ += int((4 * K * blocks[sel] + 6 * posts).sum())
    return vectors, int(blocks.sum()), bytes_, (lines if fx else None)


def main():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bf_agreement import agreement
    from ann_solo_amd import _lib, synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--library-size', type=int, default=2_100_000)
    ap.add_argument('--batch', type=int, default=32768)
    ap.add_argument('--agreement-queries', type=int, default=2048)
    ap.add_argument('--open-da', type=float, default=500.0)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default='winflat_cost.json')
    args = ap.parse_args()
    L = _lib.lib()
    dev = torch.device('cuda', 0)
    lib, aux = synthetic.make_library(args.library_size, seed=20240807, device=dev, charges=(2,), charge_p=(1.0,))
    qstep, _ = synthetic.make_queries(lib, aux, args.batch, seed=42, open_range=args.open_da, charge=2)
    qsets = {}
    for name, hard in (('default', 0.0), ('hard', synthetic.HARD_DEFAULT)):
        qsets[name], _ = synthetic.make_queries(lib, aux, args.agreement_queries, seed=43, open_range=args.open_da,
                                                charge=2, hard=hard)
    common = dict(precursor_tolerance_mass_open=args.open_da, precursor_tolerance_mode_open='Da',
                  batch_size=args.batch, seed=1234)
    out = {'library_size': lib.n, 'batch': args.batch, 'k': 1024, 'open_window_da': args.open_da,
           'steps_per_round': args.steps, 'rounds': args.rounds, 'agreement_queries': args.agreement_queries,
           'engines': {}}

    bf = SpectralLibrary(lib, config=Config.open_search(mode='bf', **common), device=dev)
    truth = {name: bf._search_batch(q, 2, 'open') for name, q in qsets.items()}      # (host outputs)
    bf.shutdown()
    print('[bf] done', flush=True)

    points = (('winflat_fp32', dict(index='winflat')),
              ('winflat_fx22', dict(index='winflat', flat_storage='fx22')),
              ('ivfflat_nprobe112', dict(index='ivfflat', num_probe=112)),
              ('ivfpq_m32_nprobe128', dict(index='ivfpq', pq_m=32, num_probe=128)))
    engines = {}
    for name, kw in points:
        t = time.perf_counter()
        sl = SpectralLibrary(lib, config=Config.open_search(mode='ann', num_list=4096, num_candidates=1024,
                                                            kmeans_niter=25, **kw, **common), device=dev)
        sl._get_ann_index(2)
        sl._search_batch(qsets['default'], 2, 'open')           # (winflat: the layout in key order is built here)
        torch.cuda.synchronize()
        engines[name] = sl
        out['engines'][name] = {'build_seconds': round(time.perf_counter() - t, 2), 'ms_per_step_rounds': []}
        print(f'[{name}] built', flush=True)

    def steps(sl, n):
        sl.set_pipeline(True)
        sl._search_batch(qstep, 2, 'open', device_out=True)
        sl.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            sl._search_batch(qstep, 2, 'open', device_out=True)
        sl.synchronize()
        dt = time.perf_counter() - t
        sl.set_pipeline(False)
        return dt / n * 1e3

    for _ in range(args.rounds):
        for name, sl in engines.items():
            out['engines'][name]['ms_per_step_rounds'].append(round(steps(sl, args.steps), 3))
    ms, n = C.c_double(), C.c_int64()
    for name, sl in engines.items():
        e = out['engines'][name]
        e['ms_per_step'] = round(float(np.mean(e['ms_per_step_rounds'])), 3)
        L.asl_profile_reset()
        L.asl_profile_enable(1)
        steps(sl, args.steps)
        L.asl_profile_enable(0)
        calls = args.steps + 1
        e['vectors_scanned_per_query'] = round(L.asl_profile_scanned_vectors() / (calls * args.batch), 1)
        for stage in ('scan', 'window_ranges', 'rescore'):
            L.asl_profile_get(stage.encode(), C.byref(ms), C.byref(n))
            if n.value:
                e[stage + '_ms_per_step'] = round(ms.value / n.value, 3)
        for qname, q in qsets.items():
            e['agreement_' + qname] = agreement(sl._search_batch(q, 2, 'open', want_knn=True), truth[qname])
        if name.startswith('winflat'):
            fx = name.endswith('fx22')
            assert sl._get_ann_index(2).flat_layout == (2 if fx else 1)
            vec, blocks, by, lines = ranged_work(sl, qstep, args.open_da, 2, fx)
            assert abs(vec / args.batch - e['vectors_scanned_per_query']) < 0.06, (vec / args.batch, e)   # the same runs
            e['counted'] = {'vectors_in_runs_per_query': round(vec / args.batch, 1),
                            'blocks_per_query': round(blocks / args.batch, 1), 'algorithmic_bytes_per_step': by,
                            'achieved_TB_per_s': round(by / e['scan_ms_per_step'] / 1e9, 3)}
            if lines is not None:
                e['counted'].update(lines_per_query=round(lines / args.batch, 1),
                                    fetched_TB_per_s_if_every_line_came_from_memory=round(
                                        lines * 128 / e['scan_ms_per_step'] / 1e9, 3))
        print(f'[{name}] {e}', flush=True)

    # IVF-Flat's own work, from its accounting kernel over a sample of the batch
    flat = engines['ivfflat_nprobe112']
    sample = qstep.select(torch.arange(2048, device=dev))
    by, lines = flat._get_ann_index(2).postings_work(flat._encode(sample), 112)
    e = out['engines']['ivfflat_nprobe112']
    e['counted'] = {'algorithmic_bytes_per_step': int(by / 2048 * args.batch), 'lines_per_query': round(lines / 2048, 1),
                    'achieved_TB_per_s': round(by / 2048 * args.batch / e['scan_ms_per_step'] / 1e9, 3),
                    'sample_queries': 2048}
    for sl in engines.values():
        sl.shutdown()

    # winflat at k 256: agreement alone
    sl = SpectralLibrary(lib, config=Config.open_search(mode='ann', index='winflat', num_candidates=256, **common),
                         device=dev)
    e = out['engines']['winflat_fp32_k256'] = {}
    for qname, q in qsets.items():
        e['agreement_' + qname] = agreement(sl._search_batch(q, 2, 'open', want_knn=True), truth[qname])
    sl.shutdown()
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
