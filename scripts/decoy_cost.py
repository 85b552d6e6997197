"""What the device decoy generator costs: spectra per second of one ``asl_decoy_batch`` call over 32 768
library spectra (about 100 peaks each, precursor charges 2 and 3, 10 ppm) for peptides of 10, 25 and 50
residues, and -- on 2 000 of the same spectra -- the time of the numpy restatement tests/decoy_ref.py.
Writes profiles/decoy_cost.json. A record, not a gate.

The numpy restatement is the only CPU baseline at hand: it is NOT the reference's
``decoy_generator.shuffle_and_reposition`` (per-spectrum spectrum_utils annotation in Python), which is
not installed here and was not timed.

    python scripts/decoy_cost.py [--out profiles/decoy_cost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N_BATCH, N_DISTINCT, N_CPU, REPEATS = 32768, 2048, 2000, 5
TOL, UNIT = 10.0, 'ppm'


def main():
    import torch
    import decoy_cases as DC
    from ann_solo_amd import decoy_generator as dg
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'decoy_cost.json'))
    args = ap.parse_args()
    runs = []
    for L in (10, 25, 50):
        rng = np.random.default_rng(L)
        distinct = [DC.make_case(rng, L, 2 + (i & 1), int(rng.integers(60, 141)), TOL, UNIT)
                    for i in range(N_DISTINCT)]
        cases = distinct * (N_BATCH // N_DISTINCT)          # the batch: every distinct spectrum 16 times
        raw, *rest = DC.pack_cases(cases)
        raw = raw.to('cuda')
        out = dg.decoy_batch(raw, *rest, TOL, UNIT, 'cuda')  # warm-up (and the answer that is checked below)
        torch.cuda.synchronize()
        times = []
        for _ in range(REPEATS):
            t = time.perf_counter()
            dg.decoy_batch(raw, *rest, TOL, UNIT, 'cuda')
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        t = time.perf_counter()
        refs = DC.reference(cases[:N_CPU], TOL, UNIT)
        t_cpu = time.perf_counter() - t
        host = {k: v.cpu().numpy() for k, v in out.items()}
        DC.assert_same(host, refs, raw.offsets.cpu().numpy(), L)   # the timed call computes the restatement's bits
        runs.append(dict(residues=L, spectra=N_BATCH, distinct_spectra=N_DISTINCT, peaks=int(raw.mz.numel()),
                         annotated_fraction=round(float((host['ann_type'] > 0).mean()), 4),
                         batch_call_s=dict(min=round(min(times), 5), mean=round(float(np.mean(times)), 5),
                                           max=round(max(times), 5)),
                         spectra_per_s=round(N_BATCH / min(times)),
                         numpy_restatement=dict(spectra=N_CPU, seconds=round(t_cpu, 3),
                                                spectra_per_s=round(N_CPU / t_cpu, 1))))
        print(json.dumps(runs[-1]), flush=True)
    doc = dict(what='asl_decoy_batch: one call over 32 768 raw library spectra (peaks on the device, peptide '
                    'arrays on the host), wall time around the call with a device synchronisation',
               tolerance=TOL, unit=UNIT, repeats=REPEATS, device=torch.cuda.get_device_name(0), runs=runs,
               note='numpy_restatement is tests/decoy_ref.py on one CPU core, the only CPU baseline here; it '
                    "is not the reference's decoy_generator (spectrum_utils), which was not measured")
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
