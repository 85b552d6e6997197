"""What the modification localisation costs: SSMs per second of one ``asl_localize_batch`` call over 32 768
SSMs (query spectra of about 50 peaks, 0.02 Da) for peptides of 10, 25 and 50 residues at precursor charges
2 and 3 (fragment charges up to 1 and 2), timed five times each, and the time of the numpy restatement
tests/localize_ref.py on the batch's 2 048 distinct inputs (the batch holds each 16 times). Writes
profiles/localize_cost.json. A record, not a gate: no speed figure was fixed in advance.

The numpy restatement on one CPU core is the only CPU baseline at hand; it is brute force over all peaks by
design and no tuned CPU implementation.

    python scripts/localize_cost.py [--out profiles/localize_cost.json]
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

N_BATCH, N_DISTINCT, REPEATS = 32768, 2048, 5
TOL, UNIT = 0.02, 'Da'


def main():
    import torch
    import localize_cases as LC
    from ann_solo_amd import localize as lz
    from ann_solo_amd.decoy_generator import default_fragment_charge
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'localize_cost.json'))
    args = ap.parse_args()
    runs = []
    for L in (10, 25, 50):
        for Z in (2, 3):
            rng = np.random.default_rng(10 * L + Z)
            distinct = [LC.random_case(rng, L, default_fragment_charge(Z), int(rng.integers(40, 61)), TOL, UNIT,
                                       LC.DELTAS[i % len(LC.DELTAS)]) for i in range(N_DISTINCT)]
            cases = distinct * (N_BATCH // N_DISTINCT)
            q, *rest = LC.pack_cases(cases)
            q = q.to('cuda')
            out = lz.localize_batch(q, *rest, TOL, UNIT, 'cuda')    # warm-up (and the answer that is checked below)
            torch.cuda.synchronize()
            times = []
            for _ in range(REPEATS):
                t = time.perf_counter()
                lz.localize_batch(q, *rest, TOL, UNIT, 'cuda')
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t)
            t = time.perf_counter()
            refs = LC.reference(distinct, TOL, UNIT)
            t_cpu = time.perf_counter() - t
            LC.assert_same(out, refs, rest[0], (L, Z))          # the timed call computes the restatement's bits
            runs.append(dict(residues=L, precursor_charge=Z, max_fragment_charge=default_fragment_charge(Z),
                             ssms=N_BATCH, distinct_ssms=N_DISTINCT, peaks=int(q.mz.numel()),
                             unique_best_site_fraction=round(float(np.mean([r['n_best'] == 1 for r in refs])), 4),
                             batch_call_s=dict(min=round(min(times), 5), mean=round(float(np.mean(times)), 5),
                                               max=round(max(times), 5), all=[round(x, 5) for x in times]),
                             ssms_per_s=round(N_BATCH / min(times)),
                             numpy_restatement=dict(ssms=N_DISTINCT, seconds=round(t_cpu, 3),
                                                    ssms_per_s=round(N_DISTINCT / t_cpu, 1))))
            print(json.dumps(runs[-1]), flush=True)
    doc = dict(what='asl_localize_batch: one call over 32 768 SSMs (query peaks on the device, peptide arrays and '
                    'deltas on the host, outputs on the device), wall time around the call with a device '
                    'synchronisation',
               tolerance=TOL, unit=UNIT, repeats=REPEATS, device=torch.cuda.get_device_name(0), runs=runs,
               note='numpy_restatement is tests/localize_ref.py on one CPU core over the 2 048 distinct inputs of '
                    'the batch, the only CPU baseline here: brute force by design, not a tuned CPU implementation')
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
