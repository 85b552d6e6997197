"""The engine's FDR step without a GPU (ann_solo_amd/fdr.py): the ``--model none`` gate is the one of
tests/fdr_gate.py bit for bit; the feature table and the scaler are the reference's; ``PercolatorTDC`` on the
numpy solver (tests/l2svm_ref.py) finds more than the cosine, falls back where it must and does not depend on
the last digits of the fitted weights; the flag, its errors, the exports."""
import argparse
import json
import logging
import os

import numpy as np
import pytest
import torch

import fdr_cases as FC
import fdr_gate
import l2svm_ref as R
from ann_solo_amd import fdr
from ann_solo_amd.config import Config, add_arguments
from ann_solo_amd.spectral_library import SSMTable
from ann_solo_amd.spectrum_similarity import FEATURE_NAMES

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------ the --model none gate
def test_gate_equals_the_test_gate_on_the_goldens():
    kat = json.load(open(os.path.join(HERE, 'golden', 'fdr_kat.json')))
    cos, decoy = np.asarray(kat['cosine']), np.asarray(kat['is_decoy'])
    np.testing.assert_array_equal(fdr.tdc_qvalues(cos, ~decoy), fdr_gate.tdc_qvalues(cos, ~decoy))
    np.testing.assert_array_equal(fdr.tdc_qvalues(cos, ~decoy, desc=False), fdr_gate.tdc_qvalues(cos, ~decoy, False))
    np.testing.assert_array_equal(np.where(decoy, np.nan, fdr.tdc_qvalues(cos, ~decoy)),
                                  np.asarray(kat['q_expected'], np.float64))
    g = np.load(os.path.join(HERE, 'golden', 'fdr_groups_golden.npz'))
    for c in range(int(g['n_cases'])):
        got = fdr.ssm_groups(g[f'md_{c}'], int(g[f'mgs_{c}']))
        np.testing.assert_array_equal(got, g[f'groups_{c}'])
        np.testing.assert_array_equal(got, fdr_gate.ssm_groups(g[f'md_{c}'], int(g[f'mgs_{c}'])))
    for n in (0, 1, 2):
        np.testing.assert_array_equal(fdr.ssm_groups(np.arange(n) * 0.3, 1), fdr_gate.ssm_groups(np.arange(n) * 0.3, 1))


@pytest.mark.parametrize('mode', ['std', 'open'])
def test_cosine_tdc_equals_the_test_gate(mode):
    a, b = FC.synthetic_table(700, 500, 3), FC.synthetic_table(700, 500, 3)
    if mode == 'open':      # mass differences that form groups
        rng = np.random.default_rng(4)
        shift = rng.choice([0.0, 15.995, 42.011, 79.966], size=len(a)) + 0.002 * rng.normal(size=len(a))
        for t in (a, b):
            for i, m in enumerate(t.query_meta[2]):
                m['precursor_mz'] = t.library_meta[2][i]['precursor_mz'] + shift[i] / 2
    mine, theirs = fdr.CosineTDC(20), fdr_gate.CosineTDC(20)
    assert mine.columnar and mine(a, mode) is None and theirs(b, mode) is None
    np.testing.assert_array_equal(a.q, b.q)
    np.testing.assert_array_equal(a.score, b.score)
    assert mine.n_groups == theirs.n_groups and (mode == 'std' or mine.n_groups > 2)


# ------------------------------------------------------------------ features and scaler
def test_feature_table_is_the_references():
    t = FC.synthetic_table(40, 30, 8)
    col = FEATURE_NAMES.index
    t.features[5, :] = np.nan                              # a query without a library row
    t.features[6, col('n_matched_peaks')] = 0              # an SSM without peak matches
    t.query_meta[2][7]['precursor_charge'] = 3
    t.query_meta[2][8]['precursor_charge'] = 6
    t.features[9, col('canberra')] = np.inf
    rows, F = fdr.feature_table(t)
    assert len(fdr.MODEL_COLUMNS) == 11 + 33 and F.shape == (68, 44) and F.dtype == np.float64
    assert list(rows) == [i for i in range(70) if i not in (5, 6)]
    assert fdr.MODEL_COLUMNS[:3] == ['sequence_len', 'precursor_charge_2', 'precursor_charge_3']
    assert fdr.MODEL_COLUMNS[11:] == list(FEATURE_NAMES)
    at = {name: F[:, k] for k, name in enumerate(fdr.MODEL_COLUMNS)}
    lm, qm = t.library_meta[2], t.query_meta[2]
    np.testing.assert_array_equal(at['sequence_len'], [len(lm[i]['peptide']) for i in rows])
    flags = np.stack([at[f'precursor_charge_{z}'] for z in (2, 3, 4, 5)], axis=1)
    assert (flags.sum(axis=1) == 1).all()
    assert flags[list(rows).index(7)].tolist() == [0, 1, 0, 0] and flags[list(rows).index(8)].tolist() == [0, 0, 0, 1]
    q = np.array([qm[i]['precursor_mz'] for i in rows])
    lp = np.array([lm[i]['precursor_mz'] for i in rows])
    np.testing.assert_array_equal(at['query_prec_mz'], q)
    np.testing.assert_array_equal(at['lib_prec_mz'], lp)
    np.testing.assert_array_equal(at['mz_diff_ppm'], (q - lp) / lp * 10 ** 6)     # spectrum_utils' mass_diff
    np.testing.assert_array_equal(at['abs_mz_diff_ppm'], np.abs(at['mz_diff_ppm']))
    np.testing.assert_array_equal(at['mz_diff_da'], q - lp)
    np.testing.assert_array_equal(at['abs_mz_diff_da'], np.abs(q - lp))
    np.testing.assert_array_equal(at['cosine'], t.features[rows, 0])
    assert np.isfinite(F).all()
    raw = t.features[rows, col('mse_mz')]
    np.testing.assert_array_equal(at['mse_mz'], np.where(np.isfinite(raw), raw, raw[np.isfinite(raw)].max()))
    fin = np.isfinite(t.features[rows, col('canberra')])
    assert at['canberra'][~fin] == t.features[rows, col('canberra')][fin].max()
    # without the columns the table cannot feed a model
    bare = t.take(np.arange(5))
    bare.features = np.zeros((5, 0))
    with pytest.raises(ValueError, match='similarity features'):
        fdr.feature_table(bare)


def test_feature_scaler_against_sklearn_and_the_reference_formula():
    pre = pytest.importorskip('sklearn.preprocessing')
    fs = pytest.importorskip('sklearn.feature_selection')
    rng = np.random.default_rng(2)
    X = rng.normal(size=(500, 6)) * [1, 10, 0.1, 3, 1, 1] + [0, 5, -2, 100, 0, 0]
    X[:, 2] = 7.25                                           # constant
    X[:, 4] = X[:, 1] * 0.3 + 0.4 * rng.normal(size=500)    # correlated at 0.99 with column 1
    assert 0.985 < np.corrcoef(X[:, 1], X[:, 4])[0, 1] < 0.995
    sc = fdr.FeatureScaler().fit(X)
    std = pre.StandardScaler().fit(X)
    np.testing.assert_allclose(sc.mean_, std.mean_, rtol=1e-14)
    np.testing.assert_allclose(sc.scale_, std.scale_, rtol=1e-14)
    Z = std.transform(X)
    vt = fs.VarianceThreshold().fit(Z)
    Zv = vt.transform(Z)
    assert vt.get_support().tolist() == [True, True, False, True, True, True]
    corr = np.abs(np.corrcoef(Zv, rowvar=False))            # CorrelationThreshold.fit (utils.py:61-62)
    mask = ~(np.tril(corr, k=-1) > 0.95).any(axis=1)
    want = np.nonzero(vt.get_support())[0][mask]
    assert np.nonzero(sc.support_)[0].tolist() == want.tolist() == [0, 1, 3, 5]
    np.testing.assert_allclose(sc.transform(X), Zv[:, mask], rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(sc.fit_transform(X), sc.transform(X))
    assert sc.transform(X).flags['C_CONTIGUOUS']
    # the same statistics from a torch tensor, computed where it lives (what the device solver's run does)
    T = torch.from_numpy(X)
    st = fdr.FeatureScaler().fit(T)
    assert st.support_.tolist() == sc.support_.tolist()
    np.testing.assert_allclose(st.mean_, sc.mean_, rtol=1e-13)
    np.testing.assert_allclose(st.scale_, sc.scale_, rtol=1e-13)
    out = st.transform(T)
    assert isinstance(out, torch.Tensor) and out.is_contiguous() and out.dtype == torch.float64
    np.testing.assert_allclose(out.numpy(), sc.transform(X), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ the Percolator-like model on the numpy solver
@pytest.fixture(scope='module')
def robust_run():
    t = FC.robust_table()
    s = fdr.PercolatorTDC(solver=R.SOLVER)
    assert s.columnar and s.uses_features and s(t, 'std') is None
    return t, s


def test_percolator_accepts_more_than_the_cosine(robust_run):
    t, s = robust_run
    c = FC.robust_table()
    fdr.CosineTDC()(c, 'std')
    n_cos, n_svm = int((c.q <= 0.01).sum()), int((t.q <= 0.01).sum())
    print(f'accepted at 1 %: cosine {n_cos}, svm {n_svm}; grid points {[tr["grid"] for tr in s.trace]}, '
          f'{s.n_fit_calls} fits')
    assert not s.fallback and 0 < n_cos < n_svm
    assert len(s.trace) == 3 and all(len(tr['labels']) == 10 == len(tr['wb']) for tr in s.trace)
    assert s.n_fit_calls == 3 * (1 + 10)          # per fold: the grid's 27 problems in one call, then 10 rounds
    decoy = t.is_decoy()
    assert np.isnan(t.q[decoy]).all() and np.isnan(t.score[decoy]).all()
    assert np.isfinite(t.q[~decoy]).all() and np.isfinite(t.score[~decoy]).all()
    # q-values are the TDC of the calibrated scores it wrote
    rows, F = fdr.feature_table(FC.robust_table())
    score, q = s.score_features(F, ~decoy[rows], F[:, fdr.MODEL_COLUMNS.index('cosine')])
    np.testing.assert_array_equal(q[~decoy], t.q[~decoy])
    np.testing.assert_array_equal(q, fdr.tdc_qvalues(score, ~decoy))
    # the held-out labels were not used: a start label of 0 outside the fold's training rows
    for tr in s.trace:
        assert 0.3 < (tr['labels'][0] == 0).mean() < 0.9 and set(np.unique(tr['labels'][-1])) == {-1, 0, 1}


def test_percolator_does_not_depend_on_the_last_digits(robust_run):
    """Every fitted weight vector moved by a random +-1e-7 (far more than the 1e-9 the two solvers may differ
    by): the same labels at every round, the same grid points, the same accepted set -- which is what lets the
    GPU test demand equality between the device solver and the numpy solver."""
    t, s = robust_run
    for seed in (5, 6):
        u = FC.robust_table()
        p = fdr.PercolatorTDC(solver=FC.perturbed(R.SOLVER, 1e-7, seed))
        p(u, 'std')
        for a, b in zip(s.trace, p.trace):
            assert a['grid'] == b['grid']
            for la, lb in zip(a['labels'], b['labels']):
                np.testing.assert_array_equal(la, lb)
        np.testing.assert_array_equal(t.q <= 0.01, u.q <= 0.01)
        fin = np.isfinite(t.score)
        assert np.abs(t.score[fin] - u.score[fin]).max() < 1e-5


def test_percolator_open_level_is_grouped():
    t = FC.synthetic_table(1500, 1500, 21)
    rng = np.random.default_rng(4)
    shift = rng.choice([0.0, 15.995, 79.966], size=len(t)) + 0.002 * rng.normal(size=len(t))
    for i, m in enumerate(t.query_meta[2]):
        m['precursor_mz'] = t.library_meta[2][i]['precursor_mz'] + shift[i] / 2
    s = fdr.PercolatorTDC(min_group_size=50, solver=R.SOLVER)
    s(t, 'open')
    assert not s.fallback and s.n_groups >= 3
    groups = fdr.ssm_groups(t.mass_diffs(), 50)
    decoy = t.is_decoy()
    rows, F = fdr.feature_table(t)
    score, q = s.score_features(F, ~decoy, F[:, 11], groups)
    for g in np.unique(groups):
        m = groups == g
        np.testing.assert_array_equal(q[m], fdr.tdc_qvalues(score[m], ~decoy[m]))
    np.testing.assert_array_equal(t.q[~decoy], q[~decoy])


def test_percolator_falls_back(caplog):
    t = FC.synthetic_table(600, 0, 9, decoys=False)
    c = FC.synthetic_table(600, 0, 9, decoys=False)
    s = fdr.PercolatorTDC(solver=R.SOLVER)
    with caplog.at_level(logging.WARNING):
        s(t, 'std')
    assert s.fallback and 'falls back' in caplog.text
    fdr.CosineTDC()(c, 'std')
    np.testing.assert_array_equal(t.q, c.q)
    np.testing.assert_array_equal(t.score, c.score)
    # a cosine on which no target passes 1 %: the same way out
    u = FC.synthetic_table(300, 300, 10)
    u.features[:, 0] = np.random.default_rng(0).random(600)
    s(u, 'std')
    assert s.fallback
    s(FC.robust_table(), 'std')
    assert not s.fallback                                    # per call


# ------------------------------------------------------------------ configuration and engine
def test_flag_and_its_errors():
    assert Config().device_fdr is False
    p = argparse.ArgumentParser()
    add_arguments(p)
    assert p.parse_args([]).device_fdr is False
    ns = p.parse_args(['--device_fdr'])
    assert ns.device_fdr is True and Config.from_reference(ns).device_fdr is True
    assert Config(device_fdr=True, model='svm', num_gpus=1).device_fdr
    assert Config(model='rf').model == 'rf'                  # carried for the caller's scorer, as ever
    with pytest.raises(ValueError, match="'none'.*'svm'"):
        Config(device_fdr=True, model='rf')
    with pytest.raises(ValueError, match='device_fdr.*sharded'):
        Config(device_fdr=True, num_gpus=2)
    assert isinstance(fdr.make_scorer(Config(device_fdr=True)), fdr.CosineTDC)
    assert isinstance(fdr.make_scorer(Config(device_fdr=True, model='none')), fdr.CosineTDC)
    s = fdr.make_scorer(Config(device_fdr=True, model='svm', fdr=0.05, fdr_min_group_size=7))
    assert isinstance(s, fdr.PercolatorTDC) and (s.fdr, s.min_group_size, s.folds, s.max_iter) == (0.05, 7, 3, 10)
    with pytest.raises(ValueError):
        fdr.make_scorer(Config(model='rf'))
    from ann_solo_amd.spectral_library import SpectralLibrary
    out = []
    for on in (False, True):                                 # no hash knows the switch
        sl = SpectralLibrary.__new__(SpectralLibrary)
        sl.config = Config.open_search(device_fdr=on)
        out.append((sl._get_hyperparameter_hash(), sl._get_index_hash()))
    assert out[0] == out[1]


def test_switch_off_is_todays_warning_path(O, monkeypatch, caplog):
    from ann_solo_amd import spectrum_similarity
    import score_hist_ref as H
    from oracle_backend import oracle_cosines
    monkeypatch.setattr(spectrum_similarity, 'ssm_cosine', oracle_cosines)
    lib, qs, qmeta, lmeta, kw = H.engine_case()
    eng = H.oracle_engine(lib, kw)
    assert eng.config.device_fdr is False
    with caplog.at_level(logging.WARNING):
        out = eng.search_packed(qs, qmeta, lmeta)
    assert 'no score_ssms callable was given' in caplog.text
    assert len(out) > 30 and (out.q == 0.0).all()
    assert out.features.shape == (len(out), 0)
    # the columns ride through take / concat / first_per_uid
    t = FC.synthetic_table(20, 10, 1)
    assert t.take(np.arange(5)).features.shape == (5, 33)
    both = SSMTable.concat([t.take(np.arange(5)), SSMTable(t.query_meta, t.library_meta), t.take([7, 9])])
    np.testing.assert_array_equal(both.features, t.features[[0, 1, 2, 3, 4, 7, 9]])
    uid = {2: np.arange(30) // 2}
    np.testing.assert_array_equal(t.first_per_uid(uid).features, t.features[::2])


def test_injected_scorer_wins_and_features_only_for_the_model(O, monkeypatch):
    """With the switch on and ``model=None`` the engine's scorer is ``CosineTDC``; an injected callable is
    called instead; only a scorer with ``uses_features`` makes the level compute the 33 columns."""
    from ann_solo_amd import spectrum_similarity
    import score_hist_ref as H
    from oracle_backend import oracle_cosines
    monkeypatch.setattr(spectrum_similarity, 'ssm_cosine', oracle_cosines)
    calls = []

    def features(q, lib, rows, pairs, count, *a):
        calls.append(a)
        F = np.full((q.n, 33), 0.5)
        F[:, 0] = oracle_cosines(q, lib, rows, pairs, count)
        return F
    monkeypatch.setattr(spectrum_similarity, 'ssm_features', features)
    lib, qs, qmeta, lmeta, kw = H.engine_case()
    eng = H.oracle_engine(lib, kw, device_fdr=True)
    eng._score_ssms = fdr.make_scorer(eng.config)           # (what SpectralLibrary.__init__ does)
    ref = H.oracle_engine(lib, kw).search_packed(qs, qmeta, lmeta, score_ssms=fdr_gate.CosineTDC(100))
    got = eng.search_packed(qs, qmeta, lmeta)
    assert not calls and len(got) == len(ref)
    for name in ('charge', 'qrow', 'lib_row', 'score', 'q'):
        np.testing.assert_array_equal(getattr(got, name), getattr(ref, name))
    seen = []

    def mine(table, mode):
        seen.append((mode, table.features.shape, table.score.copy()))
        table.q[:] = 0.0
    mine.columnar = True
    eng.search_packed(qs, qmeta, lmeta, score_ssms=mine)
    assert [m for m, _, _ in seen] == ['std', 'open'] and all(shape[1] == 0 for _, shape, _ in seen) and not calls
    mine.uses_features = True
    plain = list(seen)
    del seen[:]
    eng.search_packed(qs, qmeta, lmeta, score_ssms=mine)
    assert len(calls) >= 2
    assert all(a == (eng.config.min_mz, eng.config.max_mz, eng.config.bin_size) for a in calls)
    for (m0, _, s0), (m1, shape, s1) in zip(plain, seen):
        assert m0 == m1 and shape == (len(s1), 33)
        np.testing.assert_array_equal(s0, s1)               # the score is column 0: the same bits


# ------------------------------------------------------------------ the C ABI
def test_entry_points_are_exported():
    from ann_solo_amd import _lib
    L = _lib.lib()
    for name in ('asl_l2svm_fit', 'asl_linear_scores'):
        assert name in _lib.EXPORTS and hasattr(L, name)
    src = open(os.path.join(os.path.dirname(HERE), 'include', 'annsolo_mi.h')).read()
    assert f'#define ASL_SVM_MAX_DIM      {_lib.SVM_MAX_DIM}' in src
    assert f'#define ASL_SVM_MAX_PROBLEMS {_lib.SVM_MAX_PROBLEMS}' in src


def test_wrappers_refuse_bad_shapes():
    from ann_solo_amd import _lib
    X = np.zeros((4, 2))
    with pytest.raises(ValueError, match='label'):
        _lib.l2svm_fit(X, np.zeros((1, 5), np.int8), np.ones((1, 2)))
    with pytest.raises(ValueError, match='cw'):
        _lib.l2svm_fit(X, np.zeros((1, 4), np.int8), np.ones((2, 2)))
    with pytest.raises(ValueError, match='wb'):
        _lib.l2svm_fit(X, np.zeros((1, 4), np.int8), np.ones((1, 2)), wb=np.zeros((1, 2)))
    with pytest.raises(ValueError, match='wb'):
        _lib.linear_scores(X, np.zeros((1, 2)))
    with pytest.raises(ValueError, match='dimensions'):
        _lib.linear_scores(np.zeros(4), np.zeros((1, 2)))


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU behaviour')
def test_no_cpu_fallback():
    from ann_solo_amd import _lib
    X, lab = np.zeros((4, 2)), np.array([[1, -1, 1, -1]], np.int8)
    with pytest.raises(_lib.AnnSoloMiError, match='no HIP device'):
        _lib.l2svm_fit(X, lab, np.ones((1, 2)))
    with pytest.raises(_lib.AnnSoloMiError, match='no HIP device'):
        _lib.linear_scores(X, np.zeros((1, 3)))
    t = FC.synthetic_table(300, 300, 12)
    with pytest.raises((_lib.AnnSoloMiError, RuntimeError, AssertionError)):
        fdr.PercolatorTDC()(t, 'std')                        # the default solver is the device's: no quiet numpy


def test_limits_come_before_the_device():
    """The limits of the entry point are checked on the host before the device is asked for."""
    import ctypes as C
    from ann_solo_amd import _lib
    L = _lib.lib()
    X, lab, cw, wb = np.zeros((4, 2)), np.zeros((1, 4), np.int8), np.ones((1, 2)), np.zeros((1, 3))
    out = [np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int32)]
    par = _lib.AslL2SvmParams(1.0, 1e-9, 0.0, 10)

    def fit(n=4, d=2, P=1, par=par):
        return L.asl_l2svm_fit(_lib.ptr(X), n, d, _lib.ptr(lab), _lib.ptr(cw), P, C.byref(par), _lib.ptr(wb),
                               *[_lib.ptr(o) for o in out])
    assert fit(d=64) == -4 and fit(P=33) == -4                              # ASL_ERR_CAPACITY
    assert fit(d=0) == -1 and fit(P=0) == -1 and fit(n=-1) == -1            # ASL_ERR_INVALID
    for bad in (_lib.AslL2SvmParams(-1.0, 1e-9, 0.0, 10), _lib.AslL2SvmParams(float('nan'), 1e-9, 0.0, 10),
                _lib.AslL2SvmParams(float('inf'), 1e-9, 0.0, 10), _lib.AslL2SvmParams(1.0, -1.0, 0.0, 10),
                _lib.AslL2SvmParams(1.0, 0.0, 0.0, -1)):
        assert fit(par=bad) == -1
    assert L.asl_linear_scores(_lib.ptr(X), 4, 64, _lib.ptr(wb), 1, _lib.ptr(out[0])) == -4
    assert L.asl_linear_scores(_lib.ptr(X), 4, 2, _lib.ptr(wb), 0, _lib.ptr(out[0])) == -1
    assert b'at most 63' in L.asl_last_error() or b'needs' in L.asl_last_error()
    # the texts of the shape check the two entry points share with the forest's: no row limit is named here
    err = L.asl_last_error
    assert fit(d=64) == -4 and err() == b'l2svm_fit: d = 64, at most 63'
    assert fit(P=33) == -4 and err() == b'l2svm_fit: P = 33, at most 32'
    assert fit(n=-1) == -1 and err() == b'l2svm_fit: needs d >= 1, P >= 1, n >= 0'
    assert L.asl_linear_scores(_lib.ptr(X), 4, 2, _lib.ptr(wb), 0, _lib.ptr(out[0])) == -1
    assert err() == b'linear_scores: needs d >= 1, P >= 1, n >= 0'
    assert L.asl_linear_scores(_lib.ptr(X), 4, 2, _lib.ptr(wb), 33, _lib.ptr(out[0])) == -4
    assert err() == b'linear_scores: P = 33, at most 32'


# ------------------------------------------------------------------ an empty level, a sharded engine
@pytest.mark.parametrize('mode', ['std', 'open'])
def test_an_empty_level_is_nothing_to_score(mode, caplog):
    t = FC.synthetic_table(5, 5, 2)
    for empty in (SSMTable(t.query_meta, t.library_meta), t.take(np.zeros(0, np.int64))):   # [0, 0] and [0, 33]
        rows, F = fdr.feature_table(empty)
        assert rows.shape == (0,) and F.shape == (0, 44)
        s = fdr.PercolatorTDC(solver=R.SOLVER)
        with caplog.at_level(logging.WARNING):
            assert s(empty, mode) is None
        assert not s.fallback and 'falls back' not in caplog.text and len(empty.q) == 0 == len(empty.score)


def test_svm_engine_whose_open_level_has_no_queries_left(O, monkeypatch):
    """Level 1 identifies every query, so the open level files no batch and hands the scorer an empty table
    without feature columns: the search returns level 1's identifications."""
    from ann_solo_amd import spectrum_similarity
    import score_hist_ref as H
    from oracle_backend import oracle_cosines

    def features(q, lib, rows, pairs, count, *a):
        F = np.full((q.n, 33), 0.5)
        F[:, 0] = oracle_cosines(q, lib, rows, pairs, count)
        F[:, 2] = np.asarray(count)
        return F
    monkeypatch.setattr(spectrum_similarity, 'ssm_cosine', oracle_cosines)
    monkeypatch.setattr(spectrum_similarity, 'ssm_features', features)
    lib, qs, qmeta, lmeta, kw = H.engine_case()
    seen = []

    def first_level(table, mode):
        seen.append((mode, table.qrow.copy()))
        table.q[:] = 0.0 if mode == 'std' else 1.0
    first_level.columnar = True
    H.oracle_engine(lib, kw).search_packed(qs, qmeta, lmeta, score_ssms=first_level)
    found = seen[0][1]                                   # the queries with a standard-window match
    assert 3 < len(found) < qs[2].n
    only = {2: qs[2].select(torch.as_tensor(found))}
    meta = {2: [qmeta[2][int(i)] for i in found]}
    eng = H.oracle_engine(lib, dict(kw, fdr=0.5), device_fdr=True, model='svm')
    scorer = fdr.PercolatorTDC(0.5, 100, solver=R.SOLVER)
    levels = []

    class Spy:                                           # (the engine's own scorer, watched)
        columnar, uses_features = True, True

        def __call__(self, table, mode):
            levels.append((mode, len(table), table.features.shape))
            return scorer(table, mode)
    out = eng.search_packed(only, meta, lmeta, score_ssms=Spy())
    # no decoys in this library: level 1 falls back to the cosine, whose q = 1 / n passes at fdr = 0.5
    assert levels == [('std', len(found), (len(found), 33)), ('open', 0, (0, 0))]
    assert len(out) == len(found) and not out.open_level.any() and (out.q < 0.5).all()
    assert out.features.shape == (len(found), 33)


def test_enable_sharding_refuses_the_engines_own_scorer(monkeypatch):
    import torch.distributed as dist
    from ann_solo_amd.spectral_library import SpectralLibrary
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
    monkeypatch.setattr(dist, 'get_rank', lambda group=None: 0)
    for on in (True, False):
        sl = SpectralLibrary.__new__(SpectralLibrary)
        sl.config, sl._dist, sl.partitions = Config.open_search(device_fdr=on), None, {}
        if on:
            with pytest.raises(ValueError, match='device_fdr.*sharded'):
                sl.enable_sharding()
            assert sl._dist is None
        else:
            sl.enable_sharding()
            assert sl._dist.world == 2
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 1)
    sl = SpectralLibrary.__new__(SpectralLibrary)
    sl.config, sl._dist, sl.partitions = Config.open_search(device_fdr=True), None, {}
    sl.enable_sharding()                                 # one rank: nothing is sharded
    assert sl._dist.world == 1
