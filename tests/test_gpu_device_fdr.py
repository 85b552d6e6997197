"""The engine's FDR step on the device: ``PercolatorTDC`` with the device solver (asl_l2svm_fit /
asl_linear_scores) against the numpy solver on the table test_device_fdr_cpu.py shows to be robust, and
``Config.device_fdr`` end to end on a small library with device decoys."""
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
import l2svm_ref as R        # noqa: E402
from fake_reader import FakeReader, FakeSpectrum   # noqa: E402


def test_device_solver_equals_the_numpy_solver():
    from ann_solo_amd import fdr
    a, b = FC.robust_table(), FC.robust_table()
    dev, ref = fdr.PercolatorTDC(device='cuda:0'), fdr.PercolatorTDC(solver=R.SOLVER)
    dev(a, 'std')
    ref(b, 'std')
    assert not dev.fallback and not ref.fallback and len(dev.trace) == len(ref.trace) == 3
    for x, y in zip(dev.trace, ref.trace):
        assert x['grid'] == y['grid']
        assert len(x['labels']) == len(y['labels']) == 10
        for la, lb in zip(x['labels'], y['labels']):
            np.testing.assert_array_equal(la, lb)
        dw = max(np.abs(u - v).max() for u, v in zip(x['wb'], y['wb']))
        print('fold: grid point', x['grid'], 'max |dw| over the rounds', dw)
        assert dw <= 1e-7
    fin = np.isfinite(b.score)
    np.testing.assert_array_equal(np.isfinite(a.score), fin)
    print('max calibrated score difference', np.abs(a.score[fin] - b.score[fin]).max(),
          '; accepted at 1 %:', int((a.q <= 0.01).sum()))
    assert np.abs(a.score[fin] - b.score[fin]).max() <= 1e-6
    np.testing.assert_array_equal(a.q, b.q)
    np.testing.assert_array_equal(a.q <= 0.01, b.q <= 0.01)
    assert (a.q <= 0.01).sum() > 1500
    # the same bits from a second device run
    c = FC.robust_table()
    fdr.PercolatorTDC(device='cuda:0')(c, 'std')
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


def test_switch_off_is_todays_result(case):
    engine, qs, qmeta = case
    off = engine()
    assert off._score_ssms is None
    a = off.search_packed(qs, qmeta, off.library_meta)
    b = off.search_packed(qs, qmeta, off.library_meta, score_ssms=_Spy())
    _same(a, b)
    assert (a.q == 0.0).all() and a.features.shape == (len(a), 0) and len(a) > 500


def test_model_none_is_cosine_tdc(case):
    from ann_solo_amd import fdr
    import fdr_gate
    engine, qs, qmeta = case
    on = engine(device_fdr=True)
    assert isinstance(on._score_ssms, fdr.CosineTDC) and on._score_ssms.min_group_size == 20
    a = on.search_packed(qs, qmeta, on.library_meta)
    b = engine().search_packed(qs, qmeta, on.library_meta, score_ssms=fdr_gate.CosineTDC(20))
    _same(a, b)
    assert a.features.shape == (len(a), 0)
    assert 100 < int((a.q < 0.05).sum()) < len(a) and not a.is_decoy()[a.q < 0.05].any()
    # an injected callable wins over the switch
    spy = _Spy()
    c = on.search_packed(qs, qmeta, on.library_meta, score_ssms=spy)
    assert [m for m, _ in spy.seen] == ['std', 'open'] and (c.q == 0.0).all()


def test_model_svm_is_percolator_tdc_on_the_levels_ssms(case):
    from ann_solo_amd import fdr
    from ann_solo_amd.spectrum_similarity import FEATURE_NAMES
    engine, qs, qmeta = case
    on = engine(device_fdr=True, model='svm')
    own = on._score_ssms
    assert isinstance(own, fdr.PercolatorTDC) and (own.fdr, own.min_group_size) == (0.05, 20)
    a = on.search_packed(qs, qmeta, on.library_meta)
    # the standalone scorer, called by hand on what each level holds
    spy = _Spy(fdr.PercolatorTDC(0.05, 20, device='cuda:0'), uses_features=True)
    b = engine().search_packed(qs, qmeta, on.library_meta, score_ssms=spy)
    _same(a, b)
    np.testing.assert_array_equal(a.features, b.features)
    assert a.features.shape == (len(a), len(FEATURE_NAMES))
    std = spy.seen[0][1]
    assert spy.seen[0][0] == 'std' and std.features.shape == (len(std), 33) and std.is_decoy().any()
    rerun = fdr.PercolatorTDC(0.05, 20, device='cuda:0')
    rerun(std, 'std')
    assert not rerun.fallback                       # level 1 does train a model here
    t1 = a.take(~a.open_level)
    keep = std.q < 0.05
    np.testing.assert_array_equal(t1.q, std.q[keep])
    np.testing.assert_array_equal(t1.score, std.score[keep])
    assert 100 < keep.sum() and not std.is_decoy()[keep].any()
    # the feature columns do not change the score the gate sees: column 0 is the cosine's bits
    plain = _Spy()
    engine().search_packed(qs, qmeta, on.library_meta, score_ssms=plain)
    with_f = _Spy(uses_features=True)
    engine().search_packed(qs, qmeta, on.library_meta, score_ssms=with_f)
    for (m0, t0), (m1, t1_) in zip(plain.seen, with_f.seen):
        assert m0 == m1 and t0.features.shape[1] == 0 and t1_.features.shape[1] == 33
        assert t0.score.tobytes() == t1_.score.tobytes() == t1_.features[:, 0].tobytes()
        np.testing.assert_array_equal(t0.lib_row, t1_.lib_row)
