"""What the chimeric search costs and finds. Writes profiles/chimeric_cost.json. Records, not gates: no figure
was fixed in advance.

1. One ``asl_deplete_batch`` call (through ``chimeric.deplete_batch``: spectra on the device, outputs allocated
   on the device) over 32 768 SSMs of 50 and of 256 peaks on both sides, shifted dot product's windows at 0.02
   Da, precursor charge 2 with a +15.99 Da difference: five timed calls each, and the numpy restatement
   tests/deplete_ref.py on the batch's 2 048 distinct SSMs (whose bits the timed call must give).
2. The chimeric level on the flagship workload (BASELINE.json configs[2]: 2.1 M spectra of charge 2, IVF-PQ
   m = 32, nlist 4096, nprobe 128, 1 024 candidates) with one batch of 32 768 HARD synthetic queries
   (``synthetic.make_queries(hard=HARD_DEFAULT)``: 14.7 % of the second spectrum's level): the wall time of
   ``_chimeric_level`` on the table of the two cascade levels, and how many of the planted partners
   (``partner_row`` of the queries' truth, ``with_partner=True``) it returns. The generator draws the partner
   anywhere in the library, so only the few whose precursor happens to lie inside ``chimeric_window`` can be
   found: that number is recorded beside the hits.

    python scripts/chimeric_cost.py [--out profiles/chimeric_cost.json] [--library-size 2100000]
"""
import argparse
import json
import os
import sys
import time
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N_BATCH, N_DISTINCT, REPEATS = 32768, 2048, 5
TOL = 0.02


class LibraryMeta:
    """library_meta of a synthetic library without 2.1 M dicts: records on demand, columns from arrays."""

    def __init__(self, pmz32):
        self.pmz = pmz32

    def __len__(self):
        return len(self.pmz)

    def __getitem__(self, i):
        return dict(identifier=int(i), peptide=f'PEP{int(i)}K', precursor_mz=float(self.pmz[int(i)]))

    def column(self, name, rows):
        if name == 'precursor_mz':
            return self.pmz[rows].astype(np.float64)
        if name == 'is_decoy':
            return np.zeros(len(rows), bool)
        return [self[i][name] for i in rows]


def deplete_runs():
    import torch
    import deplete_cases as DC
    import deplete_ref as R
    from ann_solo_amd import chimeric
    from ann_solo_amd.packed import PackedSpectra
    runs = []
    for peaks in (50, 256):
        rng = np.random.default_rng(peaks)
        distinct = [DC.make_ssm(rng, peaks, peaks, 2, 15.994915, R.SCORE_SHIFT) for _ in range(N_DISTINCT)]
        q, lib, rows = DC.pack(distinct * (N_BATCH // N_DISTINCT))
        Q, L = PackedSpectra.from_numpy(*q, device='cuda'), PackedSpectra.from_numpy(*lib, device='cuda')
        d_rows = torch.from_numpy(rows).to('cuda')
        out = chimeric.deplete_batch(Q, L, d_rows, TOL, R.SCORE_SHIFT, 10, 250.0, 'cuda')      # warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(REPEATS):
            t = time.perf_counter()
            chimeric.deplete_batch(Q, L, d_rows, TOL, R.SCORE_SHIFT, 10, 250.0, 'cuda')
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        qd, ld, rd = DC.pack(distinct)
        t = time.perf_counter()
        ref = R.deplete_batch(qd, ld, rd, TOL, R.SCORE_SHIFT, 10, 250.0)
        t_cpu = time.perf_counter() - t
        # SSM s of the batch is distinct SSM s % 2048: the timed call computes the restatement's bits
        for k in ('mz', 'intensity', 'src', 'count', 'valid', 'kept_energy'):
            got = out[k].cpu().numpy().reshape((N_BATCH // N_DISTINCT, N_DISTINCT) + out[k].shape[1:])
            assert all(g.tobytes() == ref[k].astype(g.dtype).tobytes() for g in got), k
        runs.append(dict(peaks=peaks, ssms=N_BATCH, distinct_ssms=N_DISTINCT,
                         kept_fraction=round(float(ref['count'].sum()) / (peaks * N_DISTINCT), 4),
                         batch_call_s=dict(min=round(min(times), 5), mean=round(float(np.mean(times)), 5),
                                           max=round(max(times), 5), all=[round(x, 5) for x in times]),
                         ssms_per_s=round(N_BATCH / min(times)),
                         numpy_restatement=dict(ssms=N_DISTINCT, seconds=round(t_cpu, 3),
                                                ssms_per_s=round(N_DISTINCT / t_cpu, 1))))
        print(json.dumps(runs[-1]), flush=True)
    return runs


def level_run(library_size):
    import torch
    from ann_solo_amd import synthetic
    from ann_solo_amd.config import Config
    from ann_solo_amd.spectral_library import SpectralLibrary
    dev = torch.device('cuda:0')
    lib, aux = synthetic.make_library(library_size, seed=20240807, device=dev, charges=(2,), charge_p=(1.0,))
    cfg = Config.open_search(num_list=4096, num_probe=128, num_candidates=1024, index='ivfpq', pq_m=32,
                             kmeans_niter=25, mode='ann', precursor_tolerance_mass_open=500.0,
                             precursor_tolerance_mode_open='Da', batch_size=N_BATCH, seed=1234)
    sl = SpectralLibrary(lib, config=cfg, device=dev)
    q, truth = synthetic.make_queries(lib, aux, N_BATCH, seed=42, open_range=500.0, charge=2,
                                      hard=synthetic.HARD_DEFAULT, with_partner=True)
    q_pmz = q.precursor_mz.cpu().numpy()
    qmeta = {2: [dict(identifier=f'scan={i}', index=i, precursor_charge=2, precursor_mz=float(q_pmz[i]))
                 for i in range(q.n)]}
    lmeta = {2: LibraryMeta(lib.precursor_mz.cpu().numpy().astype(np.float32))}
    qs = {2: q}
    table = sl.search_packed(qs, qmeta, lmeta)             # the two cascade levels: no scorer, every SSM accepted
    torch.cuda.synchronize()
    sl.config = replace(cfg, chimeric_search=True)
    times, out = [], None
    for _ in range(3):
        sl.level_seconds = {}
        t = time.perf_counter()
        out = sl._chimeric_level(table, qs, qmeta, lmeta, None, None, len(table))
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t, sl.level_seconds.get('chimeric', (0.0, 0, 0))))
    sl.level_seconds = None
    r1 = out.chimeric_rank == 1
    partner = truth['partner_row'].cpu().numpy()
    l_pmz = lib.precursor_mz.cpu().numpy().astype(np.float32).astype(np.float64)
    primary = {int(a): int(b) for a, b in zip(table.qrow, table.lib_row)}
    in_window = np.abs(l_pmz[partner] - q_pmz) <= cfg.chimeric_window / 2.0
    # (a partner that IS the primary match cannot come back: its peptide is dropped)
    findable = in_window & np.array([primary.get(i, -1) != partner[i] for i in range(q.n)])
    hits = int(sum(partner[int(a)] == int(b) for a, b in zip(out.qrow[r1], out.lib_row[r1])))
    src = truth['source_row'].cpu().numpy()
    rec = dict(library=lib.n, queries=q.n, hard=synthetic.HARD_DEFAULT,
               levers=synthetic.hard_levers(synthetic.HARD_DEFAULT),
               chimeric_window=cfg.chimeric_window, primary_ssms=len(table),
               primary_is_source=int(sum(src[int(a)] == int(b) for a, b in zip(table.qrow, table.lib_row))),
               residues_searched=int(times[-1][1][1]), rank1_ssms=int(r1.sum()),
               explained_intensity_mean=round(float(np.nanmean(out.explained_intensity)), 4) if r1.any() else None,
               partners_planted=int((partner >= 0).sum()), partners_inside_window=int(in_window.sum()),
               partners_findable=int(findable.sum()), partners_returned=hits,
               level_wall_s=dict(all=[round(t, 4) for t, _ in times], min=round(min(t for t, _ in times), 4)),
               residue_search_wall_s=[round(a[0], 4) for _, a in times])
    print(json.dumps(rec), flush=True)
    sl.shutdown()
    return rec


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'chimeric_cost.json'))
    ap.add_argument('--library-size', type=int, default=2_100_000)
    args = ap.parse_args()
    doc = dict(what='asl_deplete_batch: one call over 32 768 SSMs (spectra, rows and outputs on the device), wall time '
                    'around chimeric.deplete_batch with a device synchronisation; the chimeric level: wall time of '
                    'SpectralLibrary._chimeric_level (depletion, packing, residue search, cosine, table) on one '
                    'batch of hard synthetic queries at configs[2]',
               tolerance=TOL, unit='Da', repeats=REPEATS, device=torch.cuda.get_device_name(0),
               deplete=deplete_runs(), level=level_run(args.library_size),
               note='numpy_restatement is tests/deplete_ref.py on one CPU core, brute force over every (query peak, '
                    'library peak, shift) by design: the only CPU baseline here, no tuned implementation. The '
                    "synthetic generator draws a query's co-fragmented partner anywhere in the library; the level "
                    'searches the isolation window only, so partners_findable is the ceiling of partners_returned.')
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
