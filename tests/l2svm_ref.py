"""The method of ``asl_l2svm_fit`` (include/annsolo_mi.h, csrc/l2svm.hip) restated in numpy: the same
objective, the same stop rule, the same Armijo constants -- and nothing of its data flow (no tiles, no
blocks, no partial sums). The GPU tests compare the kernel with it, and ``PercolatorTDC(solver=SOLVER)``
runs the package's FDR procedure on it, so a device run and a numpy run share every line of host logic.

Per problem p, over w in R^d and b (w~ = (w, b), x~ = (x, 1)):

    f = 0.5 * w~.w~ + C * sum_i cw[p, cls(i)] * max(0, 1 - y_i * w~.x~_i)^2      (y_i = label[p, i] != 0)

which is ``LinearSVC(penalty='l2', loss='squared_hinge', dual=False, fit_intercept=True,
intercept_scaling=1, C=C, class_weight={-1: cw[p, 0], +1: cw[p, 1]})``. Generalised Newton: g = w~ - 2 C sum
cw y m x~ and H = I + 2 C sum cw x~ x~^T over the rows with m = 1 - y w~.x~ > 0; H s = -g; the first t in 1,
1/2 .. 2^-7 with f(w~ + t s) <= f(w~) + 1e-4 t g.s; stop when ||g|| <= max(gtol_abs, gtol_rel * ||g0||)."""
import numpy as np

STEPS = tuple(2.0 ** -k for k in range(8))
ARMIJO = 1e-4


def objective(Z, y, c, w, C):
    m = 1.0 - y * (Z @ w)
    return 0.5 * float(w @ w) + C * float(np.sum(c * np.maximum(m, 0.0) ** 2))


def fit_one(Z, y, c, w, C, gtol_abs, gtol_rel, max_newton):
    """One problem over its own rows: ``Z [m, d + 1]`` (last column ones), ``y`` in {+1, -1}, ``c`` the rows'
    class weights, ``w`` the start. Returns (w~, objective, Newton steps, status)."""
    w = np.array(w, np.float64)
    D = Z.shape[1]
    g0, steps = None, 0
    while True:
        m = 1.0 - y * (Z @ w)
        a = m > 0
        Za, ca, ya, ma = Z[a], c[a], y[a], m[a]
        f = 0.5 * float(w @ w) + C * float(np.sum(ca * ma * ma))
        g = w - 2.0 * C * (Za.T @ (ca * ya * ma))
        gn = float(np.sqrt(g @ g))
        g0 = gn if g0 is None else g0
        if gn <= max(gtol_abs, gtol_rel * g0):
            return w, f, steps, 0
        if steps >= max_newton:
            return w, f, steps, 1
        H = np.eye(D) + 2.0 * C * ((Za.T * ca) @ Za)
        L = np.linalg.cholesky(H)
        s = np.linalg.solve(L.T, np.linalg.solve(L, -g))
        gs = float(g @ s)
        f_zero = objective(Z, y, c, w, C)
        for t in STEPS:
            if objective(Z, y, c, w + t * s, C) <= f_zero + ARMIJO * t * gs:
                break
        else:
            return w, f, steps, 2
        w = w + t * s
        steps += 1


def l2svm_fit(X, label, cw, C=1.0, gtol_abs=1e-9, gtol_rel=0.0, max_newton=100, wb=None):
    """The signature and the results of ``ann_solo_amd._lib.l2svm_fit``."""
    X = np.asarray(X, np.float64)
    label = np.asarray(label, np.int8)
    cw = np.asarray(cw, np.float64)
    n, d = X.shape
    P = label.shape[0]
    if label.shape != (P, n) or cw.shape != (P, 2):
        raise ValueError('label [P, n] and cw [P, 2] expected')
    if np.any((label < -1) | (label > 1)):
        raise ValueError('labels must be in {-1, 0, +1}')
    wb = np.zeros((P, d + 1)) if wb is None else np.array(wb, np.float64)
    Xt = np.hstack([X, np.ones((n, 1))])
    obj, steps, status = np.zeros(P), np.zeros(P, np.int32), np.zeros(P, np.int32)
    for p in range(P):
        rows = label[p] != 0
        y = label[p][rows].astype(np.float64)
        c = np.where(y > 0, cw[p, 1], cw[p, 0])
        wb[p], obj[p], steps[p], status[p] = fit_one(Xt[rows], y, c, wb[p], C, gtol_abs, gtol_rel, max_newton)
    return wb, obj, steps, status


def linear_scores(X, wb):
    """``ann_solo_amd._lib.linear_scores``: [P, n]."""
    X = np.asarray(X, np.float64)
    wb = np.asarray(wb, np.float64)
    return wb[:, :-1] @ X.T + wb[:, -1:]


#: what ``PercolatorTDC(solver=...)`` takes
SOLVER = (l2svm_fit, linear_scores)
