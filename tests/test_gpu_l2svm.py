"""asl_l2svm_fit / asl_linear_scores (csrc/l2svm.hip) against the numpy restatement tests/l2svm_ref.py, which
test_l2svm_cpu.py holds against scikit-learn. Both sides stop at ||g|| <= 1e-9 (gtol_rel = 0); H >= I then puts
each within 1e-9 of the minimiser, so 1e-7 per component leaves 50x for the rounding of the sums."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fdr_cases as FC      # noqa: E402
import l2svm_ref as R       # noqa: E402

NS, DS, PS = (1, 63, 257, 5000), (1, 15, 16, 17, 43, 63), (1, 9, 27, 32)
# every (n, d) with the problem counts taken in turn, every P at two shapes, and two runs of several tiles per
# workgroup (more than 64 rows x the CU count): sums carried over tiles in registers (P = 1, the rows of a tile
# split among the waves) and added into the workspace after every tile (P = 9)
CASES = [(n, d, PS[(i + j) % 4]) for i, n in enumerate(NS) for j, d in enumerate(DS)]
CASES += [(257, 43, P) for P in PS] + [(5000, 63, P) for P in PS] + [(5000, 16, 3), (40001, 17, 1), (40001, 17, 9)]
# the item split (by P) crossed with the Gram block count (by d) where the rotation leaves them apart
CASES += [(257, 16, 27), (257, 16, 32), (63, 63, 32), (5000, 15, 9), (63, 17, 27), (5000, 43, 9)]
CASES = sorted(set(CASES))
TOL = dict(gtol_abs=1e-9, gtol_rel=0.0, max_newton=100)


@functools.lru_cache(maxsize=None)
def reference(n, d, P):
    X, label, cw, wb0 = FC.svm_problems(n, d, P)
    return (X, label, cw, wb0), R.l2svm_fit(X, label, cw, wb=wb0, **TOL)


@pytest.mark.parametrize('n,d,P', CASES)
def test_fit_against_the_restatement(n, d, P):
    from ann_solo_amd import _lib
    (X, label, cw, wb0), (wb_r, obj_r, steps_r, status_r) = reference(n, d, P)
    assert (status_r == 0).all()
    wb, obj, steps, status = _lib.l2svm_fit(X, label, cw, wb=wb0, **TOL)
    dw = np.abs(wb - wb_r).max()
    do = np.abs(obj - obj_r) / np.maximum(np.abs(obj_r), 1e-300)
    do = np.where(obj_r == 0, np.abs(obj), do).max()
    print(f'n={n} d={d} P={P}: max |dw| = {dw:.3g}, max relative objective difference = {do:.3g}, '
          f'Newton steps {steps.min()}..{steps.max()} (restatement {steps_r.min()}..{steps_r.max()})')
    assert (status == 0).all(), status
    assert dw <= 1e-7
    assert do <= 1e-12
    if P > 1:
        assert not wb[1].any() and obj[1] == 0.0 and steps[1] == 1        # no rows, a non-zero start
    if P > 3:
        assert not wb[3].any() and steps[3] == 0                           # optimal where it starts
    # the same bits again, and with X and the labels in device memory
    again = _lib.l2svm_fit(X, label, cw, wb=wb0, **TOL)
    dev = _lib.l2svm_fit(torch.from_numpy(X).cuda(), torch.from_numpy(label).cuda(), cw, wb=wb0, **TOL)
    for other in (again, dev):
        for a, b in zip((wb, obj, steps, status), other):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('n,d,P', [(1, 1, 1), (63, 17, 9), (5000, 63, 32), (40001, 16, 3)])
def test_linear_scores(n, d, P):
    from ann_solo_amd import _lib
    rng = np.random.default_rng([n, d, P])
    X, wb = rng.normal(size=(n, d)) * 3, rng.normal(size=(P, d + 1))
    want = wb[:, :d] @ X.T + wb[:, d:]
    bound = 1e-12 * (1 + np.abs(wb[:, :d]) @ np.abs(X.T))
    got = _lib.linear_scores(X, wb)
    assert isinstance(got, np.ndarray) and got.shape == (P, n)
    assert (np.abs(got - want) <= bound).all()
    dev = _lib.linear_scores(torch.from_numpy(X).cuda(), wb)
    assert dev.is_cuda and dev.cpu().numpy().tobytes() == got.tobytes()
    assert _lib.linear_scores(np.zeros((0, d)), wb).shape == (P, 0)


def test_no_rows_at_all():
    from ann_solo_amd import _lib
    wb0 = np.arange(8, dtype=np.float64).reshape(2, 4)
    wb, obj, steps, status = _lib.l2svm_fit(np.zeros((0, 3)), np.zeros((2, 0), np.int8), np.ones((2, 2)), wb=wb0)
    assert not wb.any() and not obj.any() and steps.tolist() == [1, 1] and status.tolist() == [0, 0]


def test_iteration_cap_is_reported():
    from ann_solo_amd import _lib
    (X, label, cw, wb0), _ = reference(257, 43, 9)
    wb, obj, steps, status = _lib.l2svm_fit(X, label, cw, wb=wb0, gtol_abs=1e-9, max_newton=1)
    want = R.l2svm_fit(X, label, cw, wb=wb0, gtol_abs=1e-9, max_newton=1)
    assert status.tolist() == want[3].tolist() and 1 in status.tolist() and steps.max() == 1
    np.testing.assert_allclose(wb, want[0], atol=1e-9)


def test_limits_return_their_code_and_write_nothing():
    from ann_solo_amd import _lib
    L = _lib.lib()
    INVALID, CAPACITY = -1, -4
    X = np.random.default_rng(0).normal(size=(40, 64))
    good = np.where(np.arange(80) % 2, 1, -1).astype(np.int8).reshape(2, 40)

    def fit(n=40, d=3, P=2, label=good, cw=np.ones((2, 2)), C_=1.0, gtol=1e-9, cap=10, wb=None, device=False):
        par = _lib.AslL2SvmParams(C_, gtol, 0.0, cap)
        wb = np.full((P if 0 < P <= 32 else 2, (d if 0 < d < 64 else 3) + 1), 7.0) if wb is None else wb
        before = wb.copy()
        out = [np.full(33, 7.0), np.full(33, 7, np.int32), np.full(33, 7, np.int32)]
        lab = torch.from_numpy(label).cuda() if device else label
        rc = L.asl_l2svm_fit(_lib.ptr(X), n, d, _lib.ptr(lab), _lib.ptr(np.ascontiguousarray(cw, np.float64)), P,
                             C.byref(par), _lib.ptr(wb), *[_lib.ptr(o) for o in out])
        assert np.array_equal(wb, before, equal_nan=True) and all((o == 7).all() for o in out)
        return rc
    assert fit(d=64) == CAPACITY and fit(P=33) == CAPACITY
    assert b'at most' in L.asl_last_error()
    assert fit(d=0) == INVALID and fit(P=0) == INVALID and fit(n=-1) == INVALID
    for bad in (2, -2, 127, -128):
        lab = good.copy()
        lab[1, 39] = bad
        assert fit(label=lab) == INVALID
        assert fit(label=lab, device=True) == INVALID
    assert L.asl_last_error() == b'l2svm_fit: label[1, 39] = -128, not in {-1, 0, +1}'
    for bad in (-0.5, np.nan, np.inf, -np.inf):
        cw = np.ones((2, 2))
        cw[1, 0] = bad
        assert fit(cw=cw) == INVALID and L.asl_last_error() == b'l2svm_fit: class weights must be finite and >= 0'
        assert fit(C_=bad) == INVALID
    assert fit(gtol=-1.0) == INVALID and fit(gtol=np.nan) == INVALID and fit(cap=-1) == INVALID
    assert fit(wb=np.full((2, 4), np.nan)) == INVALID
    # the wrapper raises with the library's message; the decision function has the same limits
    with pytest.raises(_lib.AnnSoloMiError, match='label'):
        _lib.l2svm_fit(X[:, :3], (good * 2).astype(np.int8), np.ones((2, 2)))
    out = np.full(40, 7.0)
    wb = np.zeros((1, 65))
    assert L.asl_linear_scores(_lib.ptr(X), 40, 64, _lib.ptr(wb), 1, _lib.ptr(out)) == CAPACITY
    assert L.asl_linear_scores(_lib.ptr(X), 40, 3, _lib.ptr(wb), 33, _lib.ptr(out)) == CAPACITY
    assert L.asl_linear_scores(_lib.ptr(X), 40, 0, _lib.ptr(wb), 1, _lib.ptr(out)) == INVALID
    assert L.asl_linear_scores(_lib.ptr(X), -1, 3, _lib.ptr(wb), 1, _lib.ptr(out)) == INVALID
    assert (out == 7).all()
    # zero class weights and C = 0 are legal: the regulariser alone
    wb, obj, steps, status = _lib.l2svm_fit(X[:, :3], good, np.zeros((2, 2)), wb=np.ones((2, 4)))
    assert not wb.any() and not obj.any() and status.tolist() == [0, 0]
    wb, obj, steps, status = _lib.l2svm_fit(X[:, :3], good, np.ones((2, 2)), C=0.0, wb=np.ones((2, 4)))
    assert not wb.any() and status.tolist() == [0, 0]
