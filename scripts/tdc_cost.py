"""What the device q-values cost: one ``_lib.tdc_qvalues`` call on device tensors at 10^5 and 10^6 rows, ungrouped
and with 300 groups, against ``fdr.tdc_qvalues`` / ``fdr._grouped_q`` in numpy on the same arrays on the same
box; and one whole ``PercolatorTDC`` and one ``ForestTDC`` call over the synthetic tables of scripts/svm_cost.py /
forest_cost.py with ``qvalues='device'`` against ``None``. One warm-up, five timed calls each, all of them
reported. Writes profiles/tdc_cost.json. Records, not thresholds: no ratio was fixed in advance.

    python scripts/tdc_cost.py [--out profiles/tdc_cost.json] [--sizes 100000 1000000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

REPEATS = 5


def timed(fn):
    fn()                                     # warm-up: allocations, code objects, caches
    times = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return out, dict(median=round(float(np.median(times)), 5), min=round(min(times), 5), max=round(max(times), 5),
                     all=[round(t, 5) for t in times])


def main():
    import torch
    from svm_cost import table
    from ann_solo_amd import _lib, fdr
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tdc_cost.json'))
    ap.add_argument('--sizes', type=int, nargs='+', default=[100000, 1000000])
    ap.add_argument('--svm_sizes', type=int, nargs='+', default=[100000, 1000000])
    ap.add_argument('--forest_size', type=int, default=100000)
    ap.add_argument('--trees', type=int, default=100)
    args = ap.parse_args()
    calls, scorers = [], []
    for n in args.sizes:
        rng = np.random.default_rng(n)
        target = rng.random(n) < 0.5
        score = 0.45 + 0.1 * rng.normal(size=n) + 0.3 * (target & (rng.random(n) < 0.6))
        group = rng.integers(0, 300, n).astype(np.int32)
        for name, g in (('ungrouped', None), ('300_groups', group)):
            dev = [torch.as_tensor(a).cuda() for a in (score, target.astype(np.uint8))]
            gd = None if g is None else torch.as_tensor(g).cuda()

            def device():
                q = _lib.tdc_qvalues(dev[0], dev[1], gd)
                torch.cuda.synchronize()
                return q

            def host():
                return fdr.tdc_qvalues(score, target) if g is None else fdr._grouped_q(score, target, g)
            qd, td = timed(device)
            qh, th = timed(host)

            def host_arrays():               # the same call on numpy arrays: staged by the library, copied back
                return _lib.tdc_qvalues(score, target, g)
            _, ts = timed(host_arrays)
            run = dict(rows=n, groups=name, device_tensors_s=td, numpy_arrays_through_the_library_s=ts,
                       numpy_host_code_s=th, same_bytes=bool(qd.cpu().numpy().tobytes() == qh.tobytes()),
                       host_over_device_median=round(th['median'] / td['median'], 1))
            calls.append(run)
            print(json.dumps(run), flush=True)
    jobs = [('PercolatorTDC', n, lambda qv: fdr.PercolatorTDC(device='cuda:0', qvalues=qv)) for n in args.svm_sizes]
    jobs.append(('ForestTDC', args.forest_size,
                 lambda qv: fdr.ForestTDC(device='cuda:0', trees=args.trees, qvalues=qv)))
    for name, n, make in jobs:
        F, target, cos = table(n)
        run, out = dict(scorer=name, ssms=n, columns=F.shape[1]), {}
        for qv in (None, 'device'):
            s = make(qv)

            def call():
                res = s.score_features(F, target, cos)
                torch.cuda.synchronize()
                return res
            out[qv], run['qvalues_' + str(qv).lower() + '_s'] = timed(call)
        run['same_bytes'] = bool(all(a.tobytes() == b.tobytes() for a, b in zip(out[None], out['device'])))
        run['accepted_at_1pct'] = int((target & (out['device'][1] <= 0.01)).sum())
        run['none_over_device_median'] = round(run['qvalues_none_s']['median'] / run['qvalues_device_s']['median'], 2)
        scorers.append(run)
        print(json.dumps(run), flush=True)
    doc = dict(what='wall time in seconds of one call, synchronised; one warm-up and five timed calls each, all listed. '
                    'calls: _lib.tdc_qvalues on tensors resident on the device (device_tensors_s), the same entry '
                    'point on numpy arrays (staged and copied back by the library), and fdr.tdc_qvalues / '
                    'fdr._grouped_q in numpy on the same box. scorers: one score_features call (host matrix in, '
                    "scores and q-values out) with qvalues=None and qvalues='device' -- the device path copies the "
                    'score column to the device and q and the labels back on every call',
               repeats=REPEATS, device=torch.cuda.get_device_name(0), host_cpus=len(os.sched_getaffinity(0)),
               calls=calls, scorers=scorers, note='No threshold was set.')
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
