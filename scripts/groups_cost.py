"""What the device mass-difference groups cost: one ``_lib.ssm_groups`` call on a device tensor and on a numpy array
at 10^5 and 10^6 rows against ``fdr.ssm_groups`` (numpy + scipy on the host) on the same box; and, at 10^6 rows,
one grouped ``CosineTDC`` call and one ``PercolatorTDC`` open-level pass with both device switches
(``qvalues='device'``, ``groups='device'``) against ``qvalues='device'`` alone. One warm-up, five timed calls each:
medians with range, all calls listed. Writes profiles/groups_cost.json. Records, not thresholds: no ratio was
fixed in advance.

The mass differences are a mixture over -150 .. +500 Da: 40 % unmodified (0 Da, sigma 0.004), 20 % on eight
planted modification masses (sigma 0.003), 40 % uniform background. ``min_group_size`` is 100.

The scorers run on a stand-in for the level's ``SSMTable`` that holds the columns they read (the mass differences,
the decoy flags, the cosine) as arrays -- a table of 10^6 metadata dictionaries would time Python's dictionaries.
``CosineTDC`` is called as the engine calls it. ``PercolatorTDC`` is timed as the three steps its call is made of
after the feature table: the level's labels (``_level_labels``), ``score_features`` over the synthetic matrix of
scripts/svm_cost.py with those labels, and the profile (``_publish_profile``).

    python scripts/groups_cost.py [--out profiles/groups_cost.json] [--sizes 100000 1000000]
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
MIN_GROUP_SIZE = 100
MODS = (0.984, 15.9949, 42.0106, 79.9663, -17.0265, -18.0106, 1.0034, 14.0157)


def timed(fn):
    fn()                                     # warm-up: allocations, code objects, caches
    times = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return out, dict(median=round(float(np.median(times)), 5), min=round(min(times), 5), max=round(max(times), 5),
                     all=[round(t, 5) for t in times])


def mass_differences(n: int, seed: int = 1) -> np.ndarray:
    rng = np.random.default_rng([n, seed])
    kind = rng.random(n)
    md = rng.uniform(-150, 500, n)
    md[kind < 0.4] = rng.normal(0, 0.004, int((kind < 0.4).sum()))
    planted = (kind >= 0.4) & (kind < 0.6)
    md[planted] = rng.choice(np.array(MODS), int(planted.sum())) + rng.normal(0, 0.003, int(planted.sum()))
    return md


class Level:
    """The columns of an open level the scorers read."""

    def __init__(self, md, target, cosine):
        self._md, self._decoy, self._cos = md, ~target, cosine
        self.score, self.q = cosine.copy(), np.full(len(md), np.nan)

    def __len__(self):
        return len(self._md)

    def mass_diffs(self):
        return self._md

    def is_decoy(self):
        return self._decoy

    def reset(self):
        self.score = self._cos.copy()


def main():
    import torch
    from svm_cost import table
    from ann_solo_amd import _lib, fdr
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'groups_cost.json'))
    ap.add_argument('--sizes', type=int, nargs='+', default=[100000, 1000000])
    ap.add_argument('--scorer_size', type=int, default=1000000)
    args = ap.parse_args()
    calls, scorers = [], []
    for n in args.sizes:
        md = mass_differences(n)
        md_dev = torch.as_tensor(md).cuda()

        def device():
            out = _lib.ssm_groups(md_dev, MIN_GROUP_SIZE)
            torch.cuda.synchronize()
            return out

        def device_profile():
            out = _lib.ssm_groups(md_dev, MIN_GROUP_SIZE, profile=True)
            torch.cuda.synchronize()
            return out
        (gd, n_labels), td = timed(device)
        _, tp = timed(device_profile)
        _, ts = timed(lambda: _lib.ssm_groups(md, MIN_GROUP_SIZE))      # numpy arrays: staged and copied back
        gh, th = timed(lambda: fdr.ssm_groups(md, MIN_GROUP_SIZE))
        nominal = np.rint(md)
        run = dict(rows=n, intervals_occupied=int(len(np.unique(nominal))), span=int(nominal.max() - nominal.min() + 1),
                   labels=int(n_labels), device_tensor_s=td, device_tensor_with_profile_s=tp,
                   numpy_array_through_the_library_s=ts, numpy_scipy_host_code_s=th,
                   same_bytes=bool(gd.cpu().numpy().tobytes() == gh.tobytes()),
                   same_label_count=bool(n_labels == len(np.unique(gh))),
                   host_over_device_median=round(th['median'] / td['median'], 1))
        calls.append(run)
        print(json.dumps(run), flush=True)
    n = args.scorer_size
    F, target, cos = table(n)
    md = mass_differences(n)
    level = Level(md, target, cos)
    # -- CosineTDC, as the engine calls it
    run, out = dict(scorer='CosineTDC', ssms=n, mode='open'), {}
    for groups in (None, 'device'):
        s = fdr.CosineTDC(MIN_GROUP_SIZE, qvalues='device', device='cuda:0', groups=groups)

        def call():
            level.reset()
            s(level, 'open')
            torch.cuda.synchronize()
            return level.q.copy(), s.n_groups
        out[groups], run['groups_' + str(groups).lower() + '_s'] = timed(call)
    run['same_bytes'] = bool(out[None][0].tobytes() == out['device'][0].tobytes() and out[None][1] == out['device'][1])
    run['n_groups'] = int(out['device'][1])
    run['host_over_device_median'] = round(run['groups_none_s']['median'] / run['groups_device_s']['median'], 2)
    scorers.append(run)
    print(json.dumps(run), flush=True)
    # -- PercolatorTDC: the labels, score_features with them, the profile
    run, out = dict(scorer='PercolatorTDC', ssms=n, columns=F.shape[1], mode='open'), {}
    for groups in (None, 'device'):
        s = fdr.PercolatorTDC(min_group_size=MIN_GROUP_SIZE, device='cuda:0', qvalues='device', groups=groups)

        def call():
            g, _ = s._level_labels(level, 'open')
            score, q = s.score_features(F, target, cos, g)
            s._publish_profile(target, q)
            torch.cuda.synchronize()
            return score, q
        out[groups], run['groups_' + str(groups).lower() + '_s'] = timed(call)
    run['same_bytes'] = bool(all(a.tobytes() == b.tobytes() for a, b in zip(out[None], out['device'])))
    run['accepted_at_1pct'] = int((target & (out['device'][1] <= 0.01)).sum())
    run['host_over_device_median'] = round(run['groups_none_s']['median'] / run['groups_device_s']['median'], 2)
    scorers.append(run)
    print(json.dumps(run), flush=True)
    doc = dict(what='wall time in seconds of one call, synchronised; one warm-up and five timed calls each, all listed. '
                    'calls: _lib.ssm_groups on a tensor resident on the device (labels only, and with the profile '
                    'columns), the same entry point on a numpy array (staged and copied back by the library), and '
                    'fdr.ssm_groups (numpy + scipy.signal.find_peaks) on the same box. scorers: the open level with '
                    "qvalues='device' and groups=None against groups='device', at min_group_size 100 -- the device "
                    'path copies the mass differences to the device and the labels back once for the profile',
               repeats=REPEATS, min_group_size=MIN_GROUP_SIZE, device=torch.cuda.get_device_name(0),
               host_cpus=len(os.sched_getaffinity(0)), calls=calls, scorers=scorers, note='No threshold was set.')
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
