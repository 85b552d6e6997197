"""What the device FDR step costs: one ``PercolatorTDC`` call (3 folds; per fold the 27 problems of the
class-weight grid in one fit, then 10 rounds of fit / score / relabel) over synthetic feature tables of 10^5 and
10^6 SSMs x 44 columns, with the device solver (asl_l2svm_fit / asl_linear_scores) and, on the smaller table,
with the numpy solver tests/l2svm_ref.py; the device's Newton and line passes from the library's stage timers
(HIP events around the pass and the sum of its partials), with the bytes of X each pass streams; and, where
scikit-learn imports, the grid step alone as ``GridSearchCV(LinearSVC(dual=False))`` on the CPUs granted.
Writes profiles/svm_cost.json. Records, not thresholds: no speed-up was fixed in advance.

    python scripts/svm_cost.py [--out profiles/svm_cost.json] [--sizes 100000 1000000]
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))

REPEATS = 3
STAGES = ('l2svm_newton', 'l2svm_line', 'linear_scores')


def table(n, seed=1):
    """F [n, 44], is_target, cosine: half decoys; 60 % of the targets are correct and stand out a little in
    every fifth column and clearly in their sum."""
    from ann_solo_amd import fdr
    rng = np.random.default_rng(seed)
    target = rng.random(n) < 0.5
    correct = target & (rng.random(n) < 0.6)
    F = rng.normal(size=(n, len(fdr.MODEL_COLUMNS)))
    F[:, ::5] += 0.9 * correct[:, None]
    cos = fdr.MODEL_COLUMNS.index('cosine')
    F[:, cos] = 0.45 + 0.1 * rng.normal(size=n) + 0.3 * correct
    return F, target, F[:, cos].copy()


def stage_times(L):
    out = {}
    for s in STAGES:
        ms, cnt = C.c_double(0), C.c_int64(0)
        L.asl_profile_get(s.encode(), C.byref(ms), C.byref(cnt))
        out[s] = (ms.value, cnt.value)
    return out


def timed(fn, repeats):
    fn()                                     # warm-up: allocations, code objects, caches
    times = []
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return out, times


def main():
    import torch
    import l2svm_ref as R
    from ann_solo_amd import _lib, fdr
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'svm_cost.json'))
    ap.add_argument('--sizes', type=int, nargs='+', default=[100000, 1000000])
    ap.add_argument('--numpy_up_to', type=int, default=100000)
    args = ap.parse_args()
    L = _lib.lib()
    runs = []
    for n in args.sizes:
        F, target, cos = table(n)
        s = fdr.PercolatorTDC(device='cuda:0')

        def call():
            out = s.score_features(F, target, cos)
            torch.cuda.synchronize()
            return out
        (score, q), times = timed(call, REPEATS)
        run = dict(ssms=n, columns=F.shape[1], accepted_at_1pct=int((target & (q <= 0.01)).sum()),
                   columns_after_scaling=[len(tr['wb'][0]) - 1 for tr in s.trace],
                   fit_calls=s.n_fit_calls, newton_steps_longest_problem_per_call_summed=s.n_newton,
                   device_call_s=dict(min=round(min(times), 4), all=[round(t, 4) for t in times]))
        # one more call with the stage timers on
        L.asl_profile_reset()
        L.asl_profile_enable(1)
        call()
        L.asl_profile_enable(0)
        d = run['columns_after_scaling'][0]
        x_bytes = n * d * 8
        for name, (ms, cnt) in stage_times(L).items():
            if cnt:
                run[name] = dict(passes=cnt, total_ms=round(ms, 3), ms_per_pass=round(ms / cnt, 4),
                                 x_gbytes_per_s=round(x_bytes / (ms / cnt * 1e-3) / 1e9, 1))
        run['x_bytes'] = x_bytes
        run['kernel_share_of_call'] = round(sum(ms for ms, _ in stage_times(L).values()) * 1e-3 / min(times), 3)
        # the grid step alone (27 problems, one pass per step) and a single problem, timed as calls
        X = torch.as_tensor(fdr.FeatureScaler().fit_transform(F)).cuda()
        lab = np.where(target, np.where(cos > np.quantile(cos[~target], 0.99), 1, 0), -1).astype(np.int8)
        rng = np.random.default_rng(2)
        grid_lab = np.repeat(lab[None], 27, axis=0)
        grid_lab[np.arange(27)[:, None] % 3 == rng.integers(0, 3, n)[None, :]] = 0
        cw = np.array([pair for pair in fdr.GRID for _ in range(3)])
        for name, labels, weights in (('grid_27_problems', grid_lab, cw), ('one_problem', lab[None], np.ones((1, 2)))):
            def fit():
                return _lib.l2svm_fit(X, labels, weights, gtol_abs=fdr.GTOL_ABS, gtol_rel=fdr.GTOL_REL)
            (wb, obj, steps, status), t = timed(fit, REPEATS)
            run[name] = dict(seconds=round(min(t), 4), newton_steps=[int(steps.min()), int(steps.max())],
                             status=sorted(set(status.tolist())))
        if n <= args.numpy_up_to:
            ref = fdr.PercolatorTDC(solver=R.SOLVER)
            t = time.perf_counter()
            _, q_ref = ref.score_features(F, target, cos)
            run['numpy_solver_call_s'] = round(time.perf_counter() - t, 2)
            run['numpy_solver_same_accepted_set'] = bool(np.array_equal(q_ref <= 0.01, q <= 0.01))
            try:
                from sklearn.model_selection import GridSearchCV
                from sklearn.svm import LinearSVC
                rows = lab != 0
                Xh, yh = X.cpu().numpy()[rows], lab[rows]
                grid = GridSearchCV(LinearSVC(dual=False), cv=3, n_jobs=16, refit=False, param_grid=dict(
                    class_weight=[{-1: neg, 1: pos} for neg, pos in fdr.GRID]))
                t = time.perf_counter()
                grid.fit(Xh, yh)
                run['sklearn_gridsearchcv_linearsvc_s'] = round(time.perf_counter() - t, 2)
                run['sklearn_rows'] = int(rows.sum())
            except ImportError:
                pass
        runs.append(run)
        print(json.dumps(run), flush=True)
    doc = dict(what='fdr.PercolatorTDC.score_features over a synthetic feature table (host matrix in, scores and '
                    'q-values out; the scaler with torch on the device, relabelling and q-values on the host in '
                    'numpy), wall time of the call; l2svm_newton / l2svm_line / linear_scores: HIP-event time of the '
                    'passes of one further call; '
                    'x_gbytes_per_s is the size of the scaled matrix over the time of a pass',
               repeats=REPEATS, device=torch.cuda.get_device_name(0), runs=runs,
               note='grid_27_problems / one_problem: one asl_l2svm_fit call from a zero start to the stop rule of PercolatorTDC '
                    '(||g|| <= max(1e-9, 1e-13 ||g0||)), X '
                    'resident on the device. sklearn: GridSearchCV(LinearSVC(dual=False), cv=3, n_jobs=16) over the '
                    'labelled rows, default tol 1e-4 -- a looser stop than the device\'s. numpy solver: '
                    'tests/l2svm_ref.py, one process')
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
