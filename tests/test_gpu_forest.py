"""asl_forest_bin / asl_forest_fit / asl_forest_predict (csrc/forest.hip) against the numpy restatement
tests/forest_ref.py BIT FOR BIT -- every node array and every probability -- at the smallest shapes where the
kernels can go wrong; ``fdr.ForestTDC`` with the device solver against the restatement on the table
test_forest_cpu.py trains on; and ``Config.device_forest`` end to end on the small library of
test_gpu_device_fdr.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import decoy_cases as DC     # noqa: E402
import decoy_ref            # noqa: E402
import fdr_cases as FC       # noqa: E402
import forest_cases as FOC   # noqa: E402
import forest_ref as R       # noqa: E402
from fake_reader import FakeReader, FakeSpectrum   # noqa: E402

# (n, d, P, trees, depth): every n of {0, 1, 63, 64, 65, 513}, d of {1, 6, 44, 63}, P of {1, 3, 21}, trees of
# {1, 3, 16}, depth of {1, 5, 12}; 513 rows are two workgroups of the histogram pass, depth 1 runs the LDS
# histograms alone, 5 and 12 the global ones too; 21 x 16 pairs at depth 12 take several batches at the default
# workspace. binned_problems cycles the columns through 1, 2, 255 and 256 bins and holds the label edge cases.
SHAPES = [(0, 6, 3, 3, 5), (1, 1, 1, 1, 1), (63, 6, 3, 3, 5), (64, 44, 1, 16, 12), (65, 63, 3, 3, 12),
          (513, 1, 3, 1, 5), (513, 63, 1, 3, 1), (513, 6, 21, 3, 12), (513, 44, 21, 16, 12)]
FIELDS = ('col', 'bin', 'n0', 'n1', 'value')


@functools.lru_cache(maxsize=None)
def _case(n, d, P, trees, depth):
    bins, n_bins, label, cw = FOC.binned_problems(n, d, P, seed=1)
    want = R.forest_fit(bins, d, label, cw, trees=trees, max_depth=depth, seed=5, n_bins=n_bins)
    for a in (bins, n_bins, label, cw) + tuple(want.numpy().values()):
        a.setflags(write=False)
    return (bins, n_bins, label, cw), want


def _assert_same_model(got, want, what=''):
    g, w = got.numpy(), want.numpy()
    for name in FIELDS:
        assert g[name].dtype == w[name].dtype and g[name].shape == w[name].shape
        if g[name].tobytes() != w[name].tobytes():
            bad = np.argwhere(g[name] != w[name])
            raise AssertionError(f'{what}{name}: {len(bad)} nodes differ, first (p, t, node) = {bad[0].tolist()}: '
                                 f'{g[name][tuple(bad[0])]} != {w[name][tuple(bad[0])]}')


@pytest.mark.parametrize('n,d,P,trees,depth', SHAPES)
def test_fit_and_predict_equal_the_restatement(n, d, P, trees, depth):
    from ann_solo_amd import _lib
    (bins, n_bins, label, cw), want = _case(n, d, P, trees, depth)
    got = _lib.forest_fit(bins, d, label, cw, trees=trees, max_depth=depth, seed=5, n_bins=n_bins)
    assert (got.trees, got.max_depth, got.P) == (trees, depth, P)
    _assert_same_model(got, want)
    proba = _lib.forest_predict(bins, d, got)
    assert proba.shape == (P, n) and proba.tobytes() == R.forest_predict(bins, d, want).tobytes()
    if n == 0:
        assert (got.col == -1).all() and (got.value[:, :, 0] == 0.5).all()
        return
    # the same bytes from device memory, and from a second run
    dev = _lib.forest_fit(torch.tensor(bins, device='cuda'), d, torch.tensor(label, device='cuda'), cw, trees=trees,
                          max_depth=depth, seed=5, n_bins=n_bins)
    assert dev.col.is_cuda and dev.value.is_cuda
    _assert_same_model(dev, want, 'device memory: ')
    pd = _lib.forest_predict(torch.tensor(bins, device='cuda'), d, dev)
    assert pd.is_cuda and pd.cpu().numpy().tobytes() == proba.tobytes()
    _assert_same_model(_lib.forest_fit(bins, d, label, cw, trees=trees, max_depth=depth, seed=5), want, 'again: ')


def test_the_label_edge_cases_are_in_the_cases():
    (bins, n_bins, label, cw), want = _case(513, 6, 21, 3, 12)
    assert set(n_bins.tolist()) >= {1, 2, 255, 256} and (label[0] == 0).any()
    assert (label[1] == 0).all() and set(np.unique(label[2])) == {0, 1}
    rows = np.nonzero(label[3])[0]
    assert len(rows) == FOC.N_COPIES and (bins[rows] == bins[0]).all() and set(label[3, rows]) == {-1, 1}
    assert (want.value[1, :, 0] == 0.5).all() and (want.value[2, :, 0] == 1.0).all() and (want.col[3] == -1).all()
    assert cw[4, 0] == 0.0 and (want.col[0, :, 0] >= 0).all() and (want.col >= 0).sum() > 1000
    deep = np.nonzero(want.col[:, :, (1 << 11) - 1:(1 << 12) - 1] >= 0)
    assert len(deep[0]) > 0                                      # splits at the last level: leaves at level 12


def test_batches_do_not_change_the_result():
    """The 21 x 16 pairs in one batch, in three, and one pair at a time."""
    from ann_solo_amd import _lib
    n, d, P, trees, depth = 513, 44, 21, 16, 5
    (bins, n_bins, label, cw), want = _case(n, d, P, trees, depth)
    per_pair = 2 * n + (1 << (depth - 1)) * R.mtry_of(d) * 512 * 4      # a pair's node indices and histograms
    prev = _lib.set_forest_workspace(per_pair * P * trees)
    try:
        one = _lib.forest_fit(bins, d, label, cw, trees=trees, max_depth=depth, seed=5)
        assert _lib.set_forest_workspace(per_pair * (P * trees // 3)) == per_pair * P * trees
        three = _lib.forest_fit(bins, d, label, cw, trees=trees, max_depth=depth, seed=5)
        _lib.set_forest_workspace(1)
        single = _lib.forest_fit(bins, d, label, cw, trees=trees, max_depth=depth, seed=5)
    finally:
        _lib.set_forest_workspace(prev)
    for got, what in ((one, 'one batch: '), (three, 'three batches: '), (single, 'a pair per batch: ')):
        _assert_same_model(got, want, what)


def test_predict_at_every_depth_of_one_forest():
    from ann_solo_amd import _lib
    (bins, n_bins, label, cw), want = _case(513, 6, 21, 3, 12)
    got = _lib.forest_fit(bins, 6, label, cw, trees=3, max_depth=12, seed=5)
    for depth in range(13):
        assert _lib.forest_predict(bins, 6, got, depth).tobytes() == R.forest_predict(bins, 6, want, depth).tobytes()
    # a forest grown to depth 5 IS the deep one read at 5
    five = R.forest_fit(bins, 6, label, cw, trees=3, max_depth=5, seed=5)
    short = _lib.forest_fit(bins, 6, label, cw, trees=3, max_depth=5, seed=5)
    _assert_same_model(short, five)
    assert _lib.forest_predict(bins, 6, short).tobytes() == _lib.forest_predict(bins, 6, got, 5).tobytes()


@pytest.mark.parametrize('n,d', [(0, 6), (1, 1), (63, 6), (64, 44), (65, 63), (513, 44)])
def test_binning_equals_the_restatement(n, d):
    from ann_solo_amd import _lib
    X = FOC.float_matrix(n, d)
    edges, n_edges = R.bin_edges(X, np.arange(0, n, 2))
    want = R.forest_bin(X, edges, n_edges)
    got = _lib.forest_bin(X, edges, n_edges)
    assert got.dtype == np.uint8 and got.shape == (n, 64) and got.tobytes() == want.tobytes()
    if n:
        dev = _lib.forest_bin(torch.tensor(X, device='cuda'), edges, n_edges)
        assert dev.is_cuda and dev.cpu().numpy().tobytes() == want.tobytes()
        X[0, 0] = np.nan                                         # no edge is below a NaN
        assert _lib.forest_bin(X, edges, n_edges).tobytes() == R.forest_bin(X, edges, n_edges).tobytes()


def test_bad_values_are_refused_before_anything_runs():
    from ann_solo_amd import _lib
    (bins, n_bins, label, cw), _ = _case(63, 6, 3, 3, 5)
    p, i = (int(v[0]) for v in np.nonzero(label))                # the first row that carries a label
    text = r'forest_fit: label\[%d, %d\] = %d, not in \{-1, 0, \+1\}' % (p, i, 2 * label[p, i])
    with pytest.raises(_lib.AnnSoloMiError, match=text):
        _lib.forest_fit(bins, 6, (label * 2).astype(np.int8), cw, trees=1)
    with pytest.raises(_lib.AnnSoloMiError, match=text):
        _lib.forest_fit(bins, 6, torch.from_numpy((label * 2).astype(np.int8)).cuda(), cw, trees=1)
    for bad in (-1.0, np.nan, np.inf):
        w = cw.copy()
        w[1, 0] = bad
        with pytest.raises(_lib.AnnSoloMiError, match='forest_fit: class weights must be finite and >= 0'):
            _lib.forest_fit(bins, 6, label, w, trees=1)
    few = n_bins.copy()
    few[2] = 100                                                 # column 2 holds bins up to 254
    with pytest.raises(_lib.AnnSoloMiError, match='bins'):
        _lib.forest_fit(bins, 6, label, cw, trees=1, n_bins=few)
    with pytest.raises(_lib.AnnSoloMiError, match='bins'):
        _lib.forest_fit(torch.tensor(bins, device='cuda'), 6, label, cw, trees=1, n_bins=few)
    few[2] = 0
    with pytest.raises(_lib.AnnSoloMiError, match='n_bins'):
        _lib.forest_fit(bins, 6, label, cw, trees=1, n_bins=few)
    with pytest.raises(_lib.AnnSoloMiError, match='n_edges'):
        _lib.forest_bin(np.zeros((4, 2)), np.zeros((2, 255)), np.array([0, 256], np.int32))
    with pytest.raises(_lib.AnnSoloMiError, match='at most'):
        _lib.forest_fit(bins, 6, label, cw, trees=1, max_depth=13)
    # weights of zero are legal: the class then counts for nothing
    m = _lib.forest_fit(bins, 6, label, np.zeros((3, 2)), trees=2, max_depth=3, seed=5)
    assert (m.col == -1).all() and (m.value[0, :, 0] == 0.5).all() and (m.n0[0, :, 0] > 0).all()


# ------------------------------------------------------------------------------------------ ForestTDC
def test_device_solver_equals_the_restatement():
    from ann_solo_amd import fdr
    a, b = FC.robust_table(), FC.robust_table()
    dev, ref = fdr.ForestTDC(device='cuda:0', trees=16), fdr.ForestTDC(solver=R.SOLVER, trees=16)
    dev(a, 'std')
    ref(b, 'std')
    assert not dev.fallback and not ref.fallback and len(dev.trace) == len(ref.trace) == 3
    for x, y in zip(dev.trace, ref.trace):
        assert x['grid'] == y['grid'] and x['accuracy'].tobytes() == y['accuracy'].tobytes()
        assert len(x['labels']) == len(y['labels']) == 10
        for la, lb in zip(x['labels'], y['labels']):
            np.testing.assert_array_equal(la, lb)
    print('grid points', [x['grid'] for x in dev.trace], '; accepted at 1 %:', int((a.q <= 0.01).sum()))
    assert a.score.tobytes() == b.score.tobytes() and a.q.tobytes() == b.q.tobytes()
    assert (a.q <= 0.01).sum() > 1200
    assert dev.n_fit_calls == ref.n_fit_calls == 3 * (1 + 10)
    c = FC.robust_table()                                        # the same bits from a second device run
    fdr.ForestTDC(device='cuda:0', trees=16)(c, 'std')
    assert a.score.tobytes() == c.score.tobytes() and a.q.tobytes() == c.q.tobytes()


# ------------------------------------------------------------------------------------------ end to end
def _library(n=400, seed=33):
    rng = np.random.default_rng(seed)
    specs = []
    for i in range(n):
        c = DC.make_case(rng, int(rng.integers(9, 22)), 2, int(rng.integers(60, 140)), 0.02, 'Da', frac=0.8)
        mass = float(c['masses'].sum()) + decoy_ref.H2O
        specs.append(FakeSpectrum(f'lib{i:04d}', (mass + 2 * decoy_ref.PROTON) / 2, 2, c['mz'], c['intensity'], None,
                                  c['peptide'], retention_time=float(i)))
    return specs


def _queries(specs, seed=34):
    """Noisy copies of the first 300 library spectra (every third with its precursor moved by a modification
    mass, for the open level) and 300 spectra of peptides the library does not hold, at precursor masses it
    does: those match targets and decoys alike."""
    rng = np.random.default_rng(seed)
    out = []
    for j, s in enumerate(specs[:300]):
        keep = rng.random(len(s.mz)) < 0.9
        mz = np.sort((s.mz[keep] + rng.normal(0, 0.003, int(keep.sum()))).astype(np.float32))
        shift = (15.9949 if j % 3 == 0 else 0.0) / 2
        out.append(FakeSpectrum(f'scan={j}', s.precursor_mz + shift, 2, mz,
                                s.intensity[keep] * rng.uniform(0.8, 1.25, int(keep.sum())), index=j))
    for j, s in enumerate(_library(300, seed + 1)):
        host = specs[int(rng.integers(len(specs)))]
        out.append(FakeSpectrum(f'scan={300 + j}', host.precursor_mz * (1 + 2e-6 * rng.normal()), 2, s.mz, s.intensity,
                                index=300 + j))
    return out


@pytest.fixture(scope='module')
def case(tmp_path_factory):
    from ann_solo_amd.config import Config
    from ann_solo_amd.library_store import pack_queries
    from ann_solo_amd.spectral_library import SpectralLibrary
    specs = _library()
    base = dict(num_list=8, num_probe=8, num_candidates=64, kmeans_niter=4, fragment_mz_tolerance=0.02,
                decoy_tolerance_unit='Da', seed=5, min_mz_range=100.0, device_decoys=True, fdr=0.05,
                fdr_min_group_size=20, precursor_tolerance_mass=20.0, precursor_tolerance_mode='ppm')
    engines = {}

    def engine(**kw):
        key = tuple(sorted(kw.items()))
        if key not in engines:
            d = tmp_path_factory.mktemp('lib')
            reader = FakeReader(specs, str(d / 'lib.splib'))
            engines[key] = SpectralLibrary(reader, config=Config.open_search(**base, **kw), device='cuda:0')
        return engines[key]
    first = engine()
    qs, qmeta = pack_queries(iter(_queries(specs)), first.config, first.device)
    yield engine, qs, qmeta
    for e in engines.values():
        e.shutdown()


def _same(a, b):
    assert len(a) == len(b)
    for name in ('charge', 'qrow', 'lib_row', 'score', 'q', 'open_level'):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)


class _Spy:
    """A columnar scorer that keeps what every level hands it and lets ``inner`` (or nothing) decide."""
    columnar = True

    def __init__(self, inner=None, uses_features=False):
        self.inner, self.uses_features, self.seen = inner, uses_features, []

    def __call__(self, table, mode):
        self.seen.append((mode, table.take(np.arange(len(table)))))
        if self.inner is None:
            table.q[:] = 0.0
            return None
        return self.inner(table, mode)


def test_model_rf_with_the_switch_is_forest_tdc_on_the_levels_ssms(case):
    from ann_solo_amd import fdr
    from ann_solo_amd.spectrum_similarity import FEATURE_NAMES
    engine, qs, qmeta = case
    on = engine(device_fdr=True, model='rf', device_forest=True, forest_trees=16)
    own = on._score_ssms
    assert isinstance(own, fdr.ForestTDC) and (own.fdr, own.min_group_size, own.trees) == (0.05, 20, 16)
    a = on.search_packed(qs, qmeta, on.library_meta)
    # the stand-alone scorer, called by hand on what each level holds
    spy = _Spy(fdr.ForestTDC(0.05, 20, device='cuda:0', trees=16), uses_features=True)
    b = engine().search_packed(qs, qmeta, on.library_meta, score_ssms=spy)
    _same(a, b)
    np.testing.assert_array_equal(a.features, b.features)
    assert a.features.shape == (len(a), len(FEATURE_NAMES))
    std = spy.seen[0][1]
    assert spy.seen[0][0] == 'std' and std.features.shape == (len(std), 33) and std.is_decoy().any()
    rerun = fdr.ForestTDC(0.05, 20, device='cuda:0', trees=16)
    rerun(std, 'std')
    assert not rerun.fallback                       # level 1 does train a forest here
    t1 = a.take(~a.open_level)
    keep = std.q < 0.05
    np.testing.assert_array_equal(t1.q, std.q[keep])
    np.testing.assert_array_equal(t1.score, std.score[keep])
    assert 100 < keep.sum() and not std.is_decoy()[keep].any()


def test_switch_off_is_todays_search(case):
    from ann_solo_amd.config import Config
    engine, qs, qmeta = case
    off = engine()
    assert off.config.device_forest is False and off._score_ssms is None
    a = off.search_packed(qs, qmeta, off.library_meta)
    b = off.search_packed(qs, qmeta, off.library_meta, score_ssms=_Spy())
    _same(a, b)
    assert (a.q == 0.0).all() and a.features.shape == (len(a), 0) and len(a) > 500
    with pytest.raises(ValueError, match="'none'.*'svm'"):       # 'rf' alone still is not provided
        Config.open_search(device_fdr=True, model='rf')
