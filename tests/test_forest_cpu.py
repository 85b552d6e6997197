"""The device forest without a GPU: the invariants of the numpy restatement tests/forest_ref.py (which
tests/test_gpu_forest.py holds the device to, bit for bit), its agreement with scikit-learn's forest on a labelled
split, ``fdr.ForestTDC`` on the restatement, and the switch, its errors, the exports and the limits."""
import argparse
import ctypes as C
import logging
import os

import numpy as np
import pytest
import torch

import fdr_cases as FC
import forest_cases as FOC
import forest_ref as R
from ann_solo_amd import fdr
from ann_solo_amd.config import Config, add_arguments
from ann_solo_amd.spectral_library import SSMTable

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------ the restatement's invariants
@pytest.fixture(scope='module')
def grown():
    bins, n_bins, label, cw = FOC.binned_problems(513, 6, 5, seed=2)
    return (bins, n_bins, label, cw), R.forest_fit(bins, 6, label, cw, trees=4, max_depth=12, seed=9, n_bins=n_bins)


def test_the_hash_and_the_draws():
    # the finaliser is a bijection of 32-bit words that keeps 0
    assert int(R.mix(0)) == 0 and len(np.unique(R.mix(np.arange(100000)))) == 100000
    assert int(R.mix((1 << 32) + 5)) == int(R.mix(5))             # 32-bit words: the high half plays no part
    h = R.hash3(5, 2, np.arange(1000), 0)
    assert h.dtype == np.uint64 and int(h.max()) < 1 << 32 and len(np.unique(h)) == 1000
    assert not np.array_equal(h, R.hash3(6, 2, np.arange(1000), 0))
    mult = R.bootstrap(3, 4, 500)
    assert mult.shape == (4, 500) and (mult.sum(axis=1) == 500).all()
    assert 0.30 < (mult == 0).mean() < 0.44                      # about 1 / e of the rows are out of a bag
    assert not np.array_equal(mult[0], mult[1])
    for d in (1, 6, 44, 63):
        cols = R.draw_columns(3, 1, d)
        mtry = R.mtry_of(d)
        assert cols.shape == (R.NODES, mtry) and mtry == max(1, int(np.sqrt(d))) and mtry <= 7
        assert cols.min() >= 0 and cols.max() < d
        assert all(len(set(row)) == mtry for row in cols[:200].tolist())     # distinct columns per node
    first = R.draw_columns(3, 1, 44)[:, 0]
    assert len(np.unique(first)) == 44                           # every column is drawn somewhere


def test_children_sum_to_the_parent_and_the_root_is_the_bag(grown):
    (bins, n_bins, label, cw), M = grown
    mult = R.bootstrap(9, 4, len(bins))
    for p in range(label.shape[0]):
        for t in range(4):
            assert M.n0[p, t, 0] == mult[t][label[p] < 0].sum() and M.n1[p, t, 0] == mult[t][label[p] > 0].sum()
    inner = np.nonzero(M.col >= 0)
    assert len(inner[0]) > 100
    p, t, i = inner
    for side in (M.n0, M.n1):
        np.testing.assert_array_equal(side[p, t, 2 * i + 1].astype(np.int64) + side[p, t, 2 * i + 2], side[p, t, i])
    assert ((M.n0[p, t, 2 * i + 1] + M.n1[p, t, 2 * i + 1]) >= 1).all()
    assert ((M.n0[p, t, 2 * i + 2] + M.n1[p, t, 2 * i + 2]) >= 1).all()
    assert (M.n0[p, t, i] > 0).all() and (M.n1[p, t, i] > 0).all()      # a node of one class is a leaf
    assert (M.bin[p, t, i] < n_bins[M.col[p, t, i]] - 1).all()           # something goes right
    present = (M.n0.astype(np.int64) + M.n1) > 0
    w0, w1 = cw[:, 0, None, None] * M.n0, cw[:, 1, None, None] * M.n1
    with np.errstate(invalid='ignore'):
        np.testing.assert_array_equal(M.value[present & (w0 + w1 > 0)], (w1 / (w0 + w1))[present & (w0 + w1 > 0)])
    # the edge problems: no rows -> 0.5; one class -> 1; rows that no column separates -> a mixed leaf
    assert (M.col[1] == -1).all() and (M.value[1, :, 0] == 0.5).all() and (M.n0[1] == 0).all()
    assert (M.col[2] == -1).all() and (M.value[2, :, 0] == 1.0).all()
    assert (M.col[3] == -1).all() and ((M.n0[3, :, 0] > 0) | (M.n1[3, :, 0] > 0)).all()
    assert (M.col[0, :, 0] >= 0).all()


def test_a_tree_cut_at_d_is_the_tree_grown_to_d(grown):
    (bins, n_bins, label, cw), M = grown
    for depth in (1, 5):
        S = R.forest_fit(bins, 6, label, cw, trees=4, max_depth=depth, seed=9, n_bins=n_bins)
        inner, kept = (1 << depth) - 1, (1 << (depth + 1)) - 1
        np.testing.assert_array_equal(S.col[:, :, :inner], M.col[:, :, :inner])
        np.testing.assert_array_equal(S.bin[:, :, :inner], M.bin[:, :, :inner])
        assert (S.col[:, :, inner:] == -1).all() and (S.n0[:, :, kept:] == 0).all()
        for name in ('n0', 'n1', 'value'):
            assert getattr(S, name)[:, :, :kept].tobytes() == getattr(M, name)[:, :, :kept].tobytes()
        assert R.forest_predict(bins, 6, S).tobytes() == R.forest_predict(bins, 6, M, depth).tobytes()
    p0 = R.forest_predict(bins, 6, M, 0)
    np.testing.assert_array_equal(p0, np.repeat(M.value[:, :, 0].sum(axis=1, keepdims=True) / 4, len(bins), axis=1))


def test_identical_inputs_give_identical_bytes(grown):
    (bins, n_bins, label, cw), M = grown
    again = R.forest_fit(bins.copy(), 6, label.copy(), cw.copy(), trees=4, max_depth=12, seed=9, n_bins=n_bins)
    for name, a in M.numpy().items():
        assert a.tobytes() == again.numpy()[name].tobytes()
    other = R.forest_fit(bins, 6, label, cw, trees=4, max_depth=12, seed=10, n_bins=n_bins)
    assert other.col.tobytes() != M.col.tobytes()
    # a problem does not depend on its neighbours in the call
    alone = R.forest_fit(bins, 6, label[:1], cw[:1], trees=4, max_depth=12, seed=9)
    assert alone.col.tobytes() == M.col[:1].tobytes() and alone.value.tobytes() == M.value[:1].tobytes()


def test_a_duplicated_column_never_beats_its_first_copy():
    bins, n_bins, label, cw = FOC.binned_problems(513, 3, 1, seed=4)
    bins[:, 3:6] = bins[:, 0:3]                                  # columns 3 .. 5 copy 0 .. 2: d = 6, mtry = 2
    M = R.forest_fit(bins, 6, label, cw, trees=16, max_depth=12, seed=2)
    seen = 0
    for t in range(16):
        cols = R.draw_columns(2, t, 6)
        for i in np.nonzero(M.col[0, t] >= 0)[0]:
            drawn, c = cols[i].tolist(), int(M.col[0, t, i])
            twin = (c + 3) % 6
            if twin in drawn:
                seen += 1
                assert drawn.index(c) < drawn.index(twin)
    assert seen > 10


def test_binning():
    X = FOC.float_matrix(513, 6)
    train = np.arange(0, 513, 2)
    edges, n_edges = R.bin_edges(X, train)
    assert n_edges[0] == 1 and n_edges[1] == 2 and 2 < n_edges[2] < 80 and n_edges[3] == 255
    s = np.sort(X[train, 3])
    np.testing.assert_array_equal(edges[3, :255], np.unique(s[(np.arange(1, 256) * len(train)) // 256]))
    b = R.forest_bin(X, edges, n_edges)
    assert b.shape == (513, 64) and (b[:, 6:] == 0).all() and (b[:, :6].max(axis=0) <= n_edges).all()
    assert (b[:, 0] == 0).all() and set(b[:, 1]) == {0, 1} and b[:, 3].max() == 255
    for j in range(6):                                           # monotone: the order of the values is kept
        o = np.argsort(X[:, j], kind='stable')
        assert (np.diff(b[o, j].astype(int)) >= 0).all()
    assert R.forest_bin(np.array([[np.nan]]), np.zeros((1, 255)), np.array([3]))[0, 0] == 0
    mine, n_mine = fdr.forest_bin_edges(X, train)                # what ForestTDC calls: host and torch
    tor, n_tor = fdr.forest_bin_edges(torch.from_numpy(X), train)
    assert mine.tobytes() == edges.tobytes() == tor.tobytes() and n_mine.tolist() == n_edges.tolist() == n_tor.tolist()
    e0, n0 = R.bin_edges(X, np.zeros(0, np.int64))
    assert (n0 == 0).all() and (R.forest_bin(X, e0, n0) == 0).all()


# ------------------------------------------------------------------ against scikit-learn
def test_held_out_auc_against_sklearn():
    """The restatement (100 trees, depth 12) against ``RandomForestClassifier`` on the same binned matrix: its
    held-out AUC is no lower than scikit-learn's minimum over ``random_state`` 0 .. 9 minus scikit-learn's own
    spread (max - min) over those ten."""
    ens = pytest.importorskip('sklearn.ensemble')
    metrics = pytest.importorskip('sklearn.metrics')
    bins, d, n_bins, y, train, test = FOC.labelled_split()
    lab = np.zeros((1, len(y)), np.int8)
    lab[0, train] = y[train]
    M = R.forest_fit(bins, d, lab, np.ones((1, 2)), trees=100, max_depth=12, seed=FOC.AUC_SEED, n_bins=n_bins)
    mine = metrics.roc_auc_score(y[test] > 0, R.forest_predict(bins, d, M)[0, test])
    theirs = []
    for rs in range(10):
        rf = ens.RandomForestClassifier(random_state=rs, n_jobs=4).fit(bins[train, :d], y[train])
        theirs.append(metrics.roc_auc_score(y[test] > 0, rf.predict_proba(bins[test, :d])[:, 1]))
    spread = max(theirs) - min(theirs)
    print(f'held-out AUC: restatement {mine:.5f}; scikit-learn min {min(theirs):.5f} max {max(theirs):.5f} '
          f'spread {spread:.5f}')
    assert mine >= min(theirs) - spread


# ------------------------------------------------------------------ ForestTDC on the restatement
@pytest.fixture(scope='module')
def robust_run():
    t = FC.robust_table()
    s = fdr.ForestTDC(solver=R.SOLVER, trees=16)
    assert s.columnar and s.uses_features and s(t, 'std') is None
    return t, s


def test_forest_accepts_more_than_the_cosine(robust_run):
    t, s = robust_run
    c = FC.robust_table()
    fdr.CosineTDC()(c, 'std')
    n_cos, n_rf = int((c.q <= 0.01).sum()), int((t.q <= 0.01).sum())
    print(f'accepted at 1 %: cosine {n_cos}, forest {n_rf}; grid points {[tr["grid"] for tr in s.trace]}, '
          f'{s.n_fit_calls} fits')
    assert not s.fallback and 0 < n_cos < n_rf and n_rf > 1200
    assert len(s.trace) == 3 and all(len(tr['labels']) == 10 for tr in s.trace)
    assert all(0 <= tr['grid'] < 35 and tr['accuracy'].shape == (35,) for tr in s.trace)
    assert s.n_fit_calls == 3 * (1 + 10)          # per fold: the grid's 21 problems in ONE call, then 10 rounds
    decoy = t.is_decoy()
    assert np.isnan(t.q[decoy]).all() and np.isnan(t.score[decoy]).all()
    assert np.isfinite(t.q[~decoy]).all() and np.isfinite(t.score[~decoy]).all()
    for tr in s.trace:                            # the held-out part carries no label
        assert 0.3 < (tr['labels'][0] == 0).mean() < 0.9 and set(np.unique(tr['labels'][-1])) == {-1, 0, 1}


def test_the_grid_is_the_references():
    assert len(fdr.FOREST_GRID) == 35 and fdr.FOREST_GRID[0] == ((1.0, 1.0), 3) and fdr.FOREST_GRID[4][1] == 12
    assert fdr.FOREST_GRID[5] == ((0.1, 1.0), 3) and fdr.FOREST_GRID[-1] == ((10.0, 1.0), 12)
    assert [cw for cw, _ in fdr.FOREST_GRID[::5]] == [(1, 1), (.1, 1), (.1, 10), (1, .1), (1, 10), (10, .1), (10, 1)]
    calls = []
    bin_, fit, predict = R.SOLVER

    def fit_(bins, d, label, cw, **kw):
        calls.append(('fit', label.shape[0], kw['trees'], kw['max_depth']))
        return fit(bins, d, label, cw, **kw)

    def predict_(bins, d, model, max_depth=None):
        calls.append(('predict', model.P, max_depth))
        return predict(bins, d, model, max_depth)
    t = FC.synthetic_table(1500, 1500, 21)
    s = fdr.ForestTDC(fdr=0.05, solver=(bin_, fit_, predict_), trees=2, max_iter=2, folds=2)
    s(t, 'std')
    assert not s.fallback
    per_fold = len(calls) // 2
    depth = fdr.FOREST_GRID[s.trace[0]['grid']][1]
    assert calls[:per_fold] == [('fit', 21, 2, 12)] + [('predict', 21, k) for k in (3, 5, 7, 9, 12)] + \
        [('fit', 1, 2, depth), ('predict', 1, depth)] * 2
    with pytest.raises(ValueError, match='ForestTDC'):
        fdr.ForestTDC(folds=1)
    with pytest.raises(ValueError, match='PercolatorTDC'):       # the shared procedure names its model
        fdr.PercolatorTDC(max_iter=0)


def test_forest_falls_back(caplog):
    t = FC.synthetic_table(600, 0, 9, decoys=False)
    c = FC.synthetic_table(600, 0, 9, decoys=False)
    s = fdr.ForestTDC(solver=R.SOLVER, trees=2)
    with caplog.at_level(logging.WARNING):
        s(t, 'std')
    assert s.fallback and 'ForestTDC falls back' in caplog.text
    fdr.CosineTDC()(c, 'std')
    np.testing.assert_array_equal(t.q, c.q)
    np.testing.assert_array_equal(t.score, c.score)
    u = FC.synthetic_table(300, 300, 10)                         # a cosine on which no target passes 1 %
    u.features[:, 0] = np.random.default_rng(0).random(600)
    s(u, 'std')
    assert s.fallback
    v = FC.synthetic_table(300, 300, 10)
    v.features[3, 5] = np.nan                                    # (n_matched_peaks is column 2)
    s(v, 'std')
    assert s.fallback


@pytest.mark.parametrize('mode', ['std', 'open'])
def test_an_empty_level_is_nothing_to_score(mode, caplog):
    t = FC.synthetic_table(5, 5, 2)
    for empty in (SSMTable(t.query_meta, t.library_meta), t.take(np.zeros(0, np.int64))):
        s = fdr.ForestTDC(solver=R.SOLVER)
        with caplog.at_level(logging.WARNING):
            assert s(empty, mode) is None
        assert not s.fallback and 'falls back' not in caplog.text and len(empty.q) == 0 == len(empty.score)


# ------------------------------------------------------------------ the switch
def test_the_switch_and_its_errors():
    assert Config().device_forest is False and Config().forest_trees == 100
    p = argparse.ArgumentParser()
    add_arguments(p)
    ns = p.parse_args([])
    assert ns.device_forest is False and ns.forest_trees == 100
    ns = p.parse_args(['--device_fdr', '--device_forest', '--forest_trees', '16'])
    ns.model = 'rf'
    cfg = Config.from_reference(ns)
    assert cfg.device_forest is True and cfg.forest_trees == 16 and cfg.device_fdr
    cfg = Config(device_fdr=True, model='rf', device_forest=True, num_gpus=1, fdr=0.05, fdr_min_group_size=7)
    s = fdr.make_scorer(cfg)
    assert isinstance(s, fdr.ForestTDC) and s.columnar and s.uses_features
    assert (s.fdr, s.min_group_size, s.folds, s.max_iter, s.trees) == (0.05, 7, 3, 10, 100)
    assert fdr.make_scorer(Config(device_fdr=True, model='rf', device_forest=True, forest_trees=16)).trees == 16
    # its three errors
    with pytest.raises(ValueError, match='device_forest.*needs device_fdr'):
        Config(model='rf', device_forest=True)
    with pytest.raises(ValueError, match="device_forest.*model = 'rf'"):
        Config(device_fdr=True, model='svm', device_forest=True)
    with pytest.raises(ValueError, match='device_forest.*sharded'):
        Config(device_fdr=True, model='rf', device_forest=True, num_gpus=2)
    for bad in (0, -1, Config.MAX_FOREST_TREES + 1):
        with pytest.raises(ValueError, match='forest_trees'):
            Config(forest_trees=bad)
    # 'rf' alone is what it was: the old errors with their messages
    assert Config(model='rf').model == 'rf'
    with pytest.raises(ValueError, match="'none'.*'svm'"):
        Config(device_fdr=True, model='rf')
    with pytest.raises(ValueError, match="device_fdr: model = 'rf' is not provided; None / 'none' \\(cosine\\) or 'svm'"):
        fdr.make_scorer(Config(model='rf'))
    assert isinstance(fdr.make_scorer(Config(device_fdr=True, model='svm')), fdr.PercolatorTDC)
    # no hash knows the switch
    from ann_solo_amd.spectral_library import SpectralLibrary
    out = []
    for kw in (dict(), dict(device_fdr=True, model='rf', device_forest=True, forest_trees=7)):
        sl = SpectralLibrary.__new__(SpectralLibrary)
        sl.config = Config.open_search(**kw)
        out.append((sl._get_hyperparameter_hash(), sl._get_index_hash()))
    assert out[0] == out[1]


def test_enable_sharding_refuses_the_forest(monkeypatch):
    import torch.distributed as dist
    from ann_solo_amd.spectral_library import SpectralLibrary
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
    monkeypatch.setattr(dist, 'get_rank', lambda group=None: 0)
    sl = SpectralLibrary.__new__(SpectralLibrary)
    sl.config = Config.open_search(device_fdr=True, model='rf', device_forest=True)
    sl._dist, sl.partitions = None, {}
    with pytest.raises(ValueError, match='sharded'):
        sl.enable_sharding()
    assert sl._dist is None


# ------------------------------------------------------------------ the C ABI
def test_entry_points_are_exported():
    from ann_solo_amd import _lib
    L = _lib.lib()
    for name in ('asl_forest_bin', 'asl_forest_fit', 'asl_forest_predict', 'asl_set_forest_workspace'):
        assert name in _lib.EXPORTS and hasattr(L, name)
    src = open(os.path.join(os.path.dirname(HERE), 'include', 'annsolo_mi.h')).read()
    assert f'#define ASL_FOREST_MAX_BINS  {_lib.FOREST_MAX_BINS}' in src and R.MAX_BINS == _lib.FOREST_MAX_BINS
    assert f'#define ASL_FOREST_MAX_DEPTH {_lib.FOREST_MAX_DEPTH}' in src and R.MAX_DEPTH == _lib.FOREST_MAX_DEPTH
    assert f'#define ASL_FOREST_MAX_TREES {_lib.FOREST_MAX_TREES}' in src
    assert _lib.FOREST_MAX_TREES == Config.MAX_FOREST_TREES
    assert f'#define ASL_FOREST_NODES     {_lib.FOREST_NODES}' in src and R.NODES == _lib.FOREST_NODES
    assert f'#define ASL_FOREST_ROW       {_lib.FOREST_ROW}' in src and R.ROW == _lib.FOREST_ROW
    prev = _lib.set_forest_workspace(1 << 20)                     # a host-side setting: no device needed
    assert prev == 1 << 31 and _lib.set_forest_workspace(prev) == 1 << 20
    with pytest.raises(_lib.AnnSoloMiError, match='positive'):
        _lib.set_forest_workspace(0)
    assert _lib.set_forest_workspace(prev) == prev


def test_wrappers_refuse_bad_shapes():
    from ann_solo_amd import _lib
    bins = np.zeros((4, 64), np.uint8)
    with pytest.raises(ValueError, match='bins'):
        _lib.forest_fit(np.zeros((4, 6), np.uint8), 2, np.zeros((1, 4), np.int8), np.ones((1, 2)))
    with pytest.raises(ValueError, match='uint8'):
        _lib.forest_fit(np.zeros((4, 64), np.int32), 2, np.zeros((1, 4), np.int8), np.ones((1, 2)))
    with pytest.raises(ValueError, match='label'):
        _lib.forest_fit(bins, 2, np.zeros((1, 5), np.int8), np.ones((1, 2)))
    with pytest.raises(ValueError, match='cw'):
        _lib.forest_fit(bins, 2, np.zeros((1, 4), np.int8), np.ones((2, 2)))
    with pytest.raises(ValueError, match='n_bins'):
        _lib.forest_fit(bins, 2, np.zeros((1, 4), np.int8), np.ones((1, 2)), n_bins=np.ones(3))
    with pytest.raises(ValueError, match='trees'):
        _lib.forest_fit(bins, 2, np.zeros((1, 4), np.int8), np.ones((1, 2)), trees=0)
    with pytest.raises(ValueError, match='edges'):
        _lib.forest_bin(np.zeros((4, 2)), np.zeros((2, 256)), np.zeros(2, np.int32))
    with pytest.raises(ValueError, match='n_edges'):
        _lib.forest_bin(np.zeros((4, 2)), np.zeros((2, 255)), np.zeros(3, np.int32))
    with pytest.raises(ValueError, match='dimensions'):
        _lib.forest_bin(np.zeros(4), np.zeros((1, 255)), np.zeros(1, np.int32))
    with pytest.raises(ValueError, match='bins'):
        _lib.forest_predict(np.zeros((4, 63), np.uint8), 2, _lib.ForestModel(1, 1, 1))


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU behaviour')
def test_no_cpu_fallback():
    from ann_solo_amd import _lib
    bins, lab = np.zeros((4, 64), np.uint8), np.array([[1, -1, 1, -1]], np.int8)
    with pytest.raises(_lib.AnnSoloMiError, match='no HIP device'):
        _lib.forest_fit(bins, 2, lab, np.ones((1, 2)), trees=1)
    with pytest.raises(_lib.AnnSoloMiError, match='no HIP device'):
        _lib.forest_bin(np.zeros((4, 2)), np.zeros((2, 255)), np.zeros(2, np.int32))
    with pytest.raises(_lib.AnnSoloMiError, match='no HIP device'):
        _lib.forest_predict(bins, 2, _lib.ForestModel(1, 1, 1))
    t = FC.synthetic_table(300, 300, 12)
    with pytest.raises((_lib.AnnSoloMiError, RuntimeError, AssertionError)):
        fdr.ForestTDC(trees=2)(t, 'std')                         # the default solver is the device's: no quiet numpy


def test_limits_come_before_the_device():
    """The limits of the entry points are checked on the host before the device is asked for."""
    from ann_solo_amd import _lib
    L = _lib.lib()
    bins, lab, cw = np.zeros((4, 64), np.uint8), np.zeros((1, 4), np.int8), np.ones((1, 2))
    model = _lib.ForestModel(1, 1, 1)
    ms = model.struct()
    out = np.zeros((1, 4))

    def fit(n=4, d=2, P=1, trees=1, depth=1):
        par = _lib.AslForestParams(trees, depth, 1)
        return L.asl_forest_fit(_lib.ptr(bins), n, d, _lib.ptr(lab), _lib.ptr(cw), P, None, C.byref(par),
                                C.byref(ms))
    CAPACITY, INVALID = -4, -1
    assert fit(d=64) == CAPACITY and fit(P=33) == CAPACITY and fit(depth=13) == CAPACITY
    assert fit(trees=_lib.FOREST_MAX_TREES + 1) == CAPACITY
    assert b'at most' in L.asl_last_error()
    assert fit(d=0) == INVALID and fit(P=0) == INVALID and fit(n=-1) == INVALID and fit(n=1 << 31) == INVALID
    assert fit(trees=0) == INVALID and fit(depth=0) == INVALID
    # the texts of the shape check the three entry points share with the SVM's: this unit's also name the row limit
    err = L.asl_last_error
    assert fit(d=64) == CAPACITY and err() == b'forest_fit: d = 64, at most 63'
    assert fit(P=33) == CAPACITY and err() == b'forest_fit: P = 33, at most 32'
    assert fit(n=1 << 31) == INVALID and err() == b'forest_fit: needs d >= 1, P >= 1, 0 <= n < 2^31'

    def predict(n=4, d=2, P=1, depth=1):
        return L.asl_forest_predict(_lib.ptr(bins), n, d, C.byref(ms), P, depth, _lib.ptr(out))
    assert predict(d=64) == CAPACITY and predict(P=33) == CAPACITY and predict(depth=13) == CAPACITY
    assert predict(d=0) == INVALID and predict(n=-1) == INVALID and predict(depth=-1) == INVALID
    assert predict(n=-1) == INVALID and err() == b'forest_predict: needs d >= 1, P >= 1, 0 <= n < 2^31'
    assert predict(P=33) == CAPACITY and err() == b'forest_predict: P = 33, at most 32'
    assert predict(n=0) == 0                                     # nothing to do, no device asked for
    X, edges, ne = np.zeros((4, 2)), np.zeros((2, 255)), np.zeros(2, np.int32)
    ob = np.zeros((4, 64), np.uint8)
    assert L.asl_forest_bin(_lib.ptr(X), 4, 64, _lib.ptr(edges), _lib.ptr(ne), _lib.ptr(ob)) == CAPACITY
    assert L.asl_forest_bin(_lib.ptr(X), 4, 0, _lib.ptr(edges), _lib.ptr(ne), _lib.ptr(ob)) == INVALID
    assert L.asl_forest_bin(_lib.ptr(X), -1, 2, _lib.ptr(edges), _lib.ptr(ne), _lib.ptr(ob)) == INVALID
    assert err() == b'forest_bin: needs d >= 1, P >= 1, 0 <= n < 2^31'
    assert L.asl_forest_bin(_lib.ptr(X), 4, 64, _lib.ptr(edges), _lib.ptr(ne), _lib.ptr(ob)) == CAPACITY
    assert err() == b'forest_bin: d = 64, at most 63'
