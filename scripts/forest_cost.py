"""What the device forest costs: one ``ForestTDC`` call (3 folds; per fold the 21 problems of the class-weight
grid as one fit at depth 12 and five predictions, then 10 rounds of fit / predict / relabel) over a synthetic
feature table of 10^5 SSMs x 44 columns with the device solver (asl_forest_bin / asl_forest_fit /
asl_forest_predict); the grid fit and a single-problem fit alone; the passes from the library's stage timers; and,
where scikit-learn imports, ``RandomForestClassifier`` on the same binned matrix on the CPUs granted.
Writes profiles/forest_cost.json. Records, not thresholds: no speed-up was fixed in advance.

    python scripts/forest_cost.py [--out profiles/forest_cost.json] [--size 100000] [--trees 100]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

REPEATS = 3
STAGES = ('forest_bin', 'forest_draws', 'forest_hist', 'forest_split', 'forest_predict')


def stage_times(L):
    out = {}
    for s in STAGES:
        ms, cnt = C.c_double(0), C.c_int64(0)
        L.asl_profile_get(s.encode(), C.byref(ms), C.byref(cnt))
        out[s] = (ms.value, cnt.value)
    return out


def main():
    import torch
    from svm_cost import table, timed
    from ann_solo_amd import _lib, fdr
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'forest_cost.json'))
    ap.add_argument('--size', type=int, default=100000)
    ap.add_argument('--trees', type=int, default=100)
    ap.add_argument('--cpus', type=int, default=16)
    args = ap.parse_args()
    L = _lib.lib()
    n = args.size
    F, target, cos = table(n)
    s = fdr.ForestTDC(device='cuda:0', trees=args.trees)

    def call():
        out = s.score_features(F, target, cos)
        torch.cuda.synchronize()
        return out
    (score, q), times = timed(call, REPEATS)
    run = dict(ssms=n, columns=F.shape[1], trees=args.trees, accepted_at_1pct=int((target & (q <= 0.01)).sum()),
               grid_points=[tr['grid'] for tr in s.trace],
               chosen=[[list(fdr.FOREST_GRID[tr['grid']][0]), fdr.FOREST_GRID[tr['grid']][1]] for tr in s.trace],
               fit_calls_per_call=s.n_fit_calls // (REPEATS + 1),
               device_call_s=dict(min=round(min(times), 4), all=[round(t, 4) for t in times]))
    run['cosine_accepted_at_1pct'] = int((target & (fdr.tdc_qvalues(cos, target) <= 0.01)).sum())
    L.asl_profile_reset()
    L.asl_profile_enable(1)
    call()
    L.asl_profile_enable(0)
    for name, (ms, cnt) in stage_times(L).items():
        if cnt:
            run[name] = dict(launches=cnt, total_ms=round(ms, 3), ms_per_launch=round(ms / cnt, 4))
    run['kernel_share_of_call'] = round(sum(ms for ms, _ in stage_times(L).values()) * 1e-3 / min(times), 3)
    # the grid fit alone (21 problems x trees at depth 12) and one problem, timed as calls on a resident matrix
    X = torch.as_tensor(fdr.FeatureScaler().fit_transform(F)).cuda()
    d = int(X.shape[1])
    edges, n_edges = fdr.forest_bin_edges(X, np.arange(n))
    bins = _lib.forest_bin(X, edges, n_edges)
    lab = np.where(target, np.where(cos > np.quantile(cos[~target], 0.99), 1, 0), -1).astype(np.int8)
    rng = np.random.default_rng(2)
    grid_lab = np.repeat(lab[None], 21, axis=0)
    grid_lab[np.arange(21)[:, None] % 3 == rng.integers(0, 3, n)[None, :]] = 0
    cw = np.array([pair for pair in fdr.FOREST_CLASS_WEIGHTS for _ in range(3)])
    run['columns_after_scaling'] = d
    for name, labels, weights in (('grid_21_problems', grid_lab, cw), ('one_problem', lab[None], np.ones((1, 2)))):
        def fit():
            m = _lib.forest_fit(bins, d, labels, weights, trees=args.trees, max_depth=12, seed=1)
            torch.cuda.synchronize()
            return m
        model, t = timed(fit, REPEATS)
        run[name] = dict(fit_seconds=round(min(t), 4), forests=int(labels.shape[0]),
                         internal_nodes=int((model.col >= 0).sum().item()))

        def predict():
            p = _lib.forest_predict(bins, d, model)
            torch.cuda.synchronize()
            return p
        _, t = timed(predict, REPEATS)
        run[name]['predict_seconds'] = round(min(t), 4)
    try:
        from sklearn.ensemble import RandomForestClassifier
        rows = lab != 0
        Xh, yh = bins.cpu().numpy()[rows, :d], lab[rows]
        rf = RandomForestClassifier(n_estimators=args.trees, max_depth=12, n_jobs=args.cpus, random_state=1)
        t = time.perf_counter()
        rf.fit(Xh, yh)
        run['sklearn_one_forest_fit_s'] = round(time.perf_counter() - t, 2)
        t = time.perf_counter()
        rf.predict_proba(bins.cpu().numpy()[:, :d])
        run['sklearn_one_forest_predict_s'] = round(time.perf_counter() - t, 2)
        run['sklearn_rows'], run['sklearn_cpus'] = int(rows.sum()), args.cpus
    except ImportError:
        pass
    print(json.dumps(run), flush=True)
    doc = dict(what='fdr.ForestTDC.score_features over a synthetic feature table (host matrix in, scores and q-values '
                    'out; the scaler and the edge sort with torch on the device, relabelling and q-values on the '
                    'host in numpy), wall time of the call; forest_*: HIP-event time of the launches of one further '
                    'call (forest_hist includes the partition step)',
               repeats=REPEATS, device=torch.cuda.get_device_name(0), run=run,
               note='grid_21_problems / one_problem: one asl_forest_fit call at depth 12 and one asl_forest_predict '
                    'call, the binned matrix and the model resident on the device. sklearn: ONE '
                    'RandomForestClassifier(n_estimators=trees, max_depth=12, n_jobs=cpus) on the same binned '
                    "matrix's labelled rows -- the reference's grid is 105 such fits of varying depth. "
                    'No threshold was set.')
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
