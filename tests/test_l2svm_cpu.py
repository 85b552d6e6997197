"""tests/l2svm_ref.py, the numpy restatement of ``asl_l2svm_fit``'s method, against scikit-learn's
``LinearSVC(dual=False)`` (liblinear's primal trust-region Newton on the same objective): the GPU tests then
only have to compare the kernel with the restatement."""
import numpy as np
import pytest

import l2svm_ref as R

SHAPES = [(64, 3), (257, 1), (300, 7), (2000, 43), (5000, 43)]
WEIGHTS = [(1.0, 1.0), (0.1, 10.0), (10.0, 0.1)]


def _problem(n, d):
    rng = np.random.default_rng([n, d])
    X = rng.normal(size=(n, d))
    y = np.where(X @ rng.normal(size=d) + rng.normal(size=n) > 0, 1, -1).astype(np.int8)
    return X, y


@pytest.mark.parametrize('cw', WEIGHTS)
@pytest.mark.parametrize('n,d', SHAPES)
def test_restatement_against_linearsvc(n, d, cw):
    svm = pytest.importorskip('sklearn.svm')
    X, y = _problem(n, d)
    wb, obj, steps, status = R.l2svm_fit(X, y[None], np.array([cw]))
    assert status[0] == 0 and 1 <= steps[0] <= 30
    m = svm.LinearSVC(dual=False, tol=1e-12, max_iter=100000, class_weight={-1: cw[0], 1: cw[1]}).fit(X, y)
    theirs = np.append(m.coef_[0], m.intercept_[0])
    Z = np.hstack([X, np.ones((n, 1))])
    c = np.where(y > 0, cw[1], cw[0])
    f_theirs = R.objective(Z, y.astype(np.float64), c, theirs, 1.0)
    diff = np.abs(wb[0] - theirs).max()
    print(f'n={n} d={d} cw={cw}: max |dw| = {diff:.3g}, objective {obj[0]!r} vs sklearn {f_theirs!r}, '
          f'{steps[0]} Newton steps')
    assert diff <= 1e-6
    assert obj[0] <= f_theirs * (1 + 1e-12)
    assert obj[0] == pytest.approx(R.objective(Z, y.astype(np.float64), c, wb[0], 1.0), rel=1e-13)


def test_rows_labelled_zero_are_not_there():
    X, y = _problem(300, 7)
    rng = np.random.default_rng(3)
    drop = rng.random(300) < 0.3
    lab = np.where(drop, 0, y).astype(np.int8)
    cw = np.array([[0.5, 2.0]])
    a = R.l2svm_fit(X, lab[None], cw)
    b = R.l2svm_fit(X[~drop], y[~drop][None], cw)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def test_several_problems_starts_and_edges():
    X, y = _problem(257, 5)
    lab = np.stack([y, np.zeros_like(y), np.abs(y), -y]).astype(np.int8)
    cw = np.array([[1, 1], [1, 1], [2, 3], [0.1, 10.0]])
    wb0 = np.random.default_rng(1).normal(size=(4, 6))
    wb, obj, steps, status = R.l2svm_fit(X, lab, cw, wb=wb0)
    assert (status == 0).all()
    np.testing.assert_array_equal(wb[1], 0.0)            # no rows: the regulariser alone, one full step
    assert obj[1] == 0.0 and steps[1] == 1
    cold = R.l2svm_fit(X, lab, cw)
    np.testing.assert_allclose(wb, cold[0], atol=1e-8)   # the minimiser does not depend on the start
    assert cold[2][1] == 0                               # already optimal at a zero start
    s = R.linear_scores(X, wb)
    assert s.shape == (4, 257)
    np.testing.assert_allclose(s[0], X @ wb[0, :5] + wb[0, 5], rtol=1e-13, atol=1e-13)
    assert (s[2] > 0).mean() > 0.99                      # one class: everything on its side
    # iteration cap and bad labels
    assert R.l2svm_fit(X, lab[:1], cw[:1], max_newton=1)[3][0] == 1
    with pytest.raises(ValueError):
        R.l2svm_fit(X, (2 * lab[:1]).astype(np.int8), cw[:1])
