"""``asl_ssm_groups`` (csrc/groups.hip) against the host code ``fdr.ssm_groups``, byte for byte, on every case of
tests/groups_cases.py, for numpy arrays and device tensors; its errors; the three scorers with ``groups='device'``
against themselves without, with and without ``qvalues='device'``; and ``Config.device_groups`` end to end on the
small library of test_gpu_tdc.py. The tolerance is zero everywhere."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fdr_cases as FC          # noqa: E402
import groups_cases as GC       # noqa: E402
import test_gpu_tdc as TT       # noqa: E402  (its grouped table, library and queries)
from fake_reader import FakeReader   # noqa: E402

DEV = 'cuda:0'


def _on_device(a):
    return torch.as_tensor(np.array(a)).to(DEV)      # (a copy: the cases are read-only)


def _host(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else a


@pytest.mark.parametrize('name', GC.NAMES)
def test_labels_and_profile_equal_the_host_code(name):
    from ann_solo_amd import _lib
    md, min_size = GC.CASES[name]
    want = GC.host(name)
    _, n_peaks, n_labels, mass, size = GC.ref(name)
    assert n_labels == len(np.unique(want))
    for arg, kind in ((md, np.ndarray), (_on_device(md), torch.Tensor)):
        for _ in range(2):          # a second call: the same bytes (the workspace is reused)
            g, nl = _lib.ssm_groups(arg, min_size)
            assert isinstance(g, kind) and _host(g).dtype == np.int32 and (kind is np.ndarray or g.is_cuda)
            assert _host(g).tobytes() == want.tobytes() and nl == n_labels
            g, nl, pm, psz = _lib.ssm_groups(arg, min_size, profile=True)
            assert isinstance(pm, kind) and isinstance(psz, kind)
            assert _host(g).tobytes() == want.tobytes() and nl == n_labels
            assert len(pm) == len(psz) == n_peaks
            assert _host(pm).dtype == np.float64 and _host(pm).tobytes() == mass.tobytes()
            assert _host(psz).dtype == np.int64 and _host(psz).tobytes() == size.tobytes()


def _raw(md, n, min_size, group, mass=None, size=None):
    import ctypes
    from ann_solo_amd import _lib
    n_peaks, n_labels = ctypes.c_int64(-5), ctypes.c_int64(-5)
    rc = _lib.lib().asl_ssm_groups(_lib.ptr(md), n, min_size, _lib.ptr(group), ctypes.byref(n_peaks),
                                   ctypes.byref(n_labels), _lib.ptr(mass), _lib.ptr(size))
    return rc, n_peaks.value, n_labels.value


@pytest.mark.parametrize('device', [False, True])
def test_errors_leave_the_outputs_untouched(device):
    from ann_solo_amd import _lib
    rng = np.random.default_rng(4)
    n = 1500
    md = rng.normal(0, 0.01, n) + rng.integers(-3, 4, n)
    move = _on_device if device else (lambda a: a)
    g0, m0, s0 = np.full(n, 77, np.int32), np.full(n, -7.0), np.full(n, 99, np.int64)
    bad = {}
    for what, v in (('nan', np.nan), ('inf', np.inf), ('minus_inf', -np.inf)):
        bad[what] = md.copy()
        bad[what][1234] = v
    over = np.concatenate([md[:n - len(GC.OVER_SPAN)], GC.OVER_SPAN])
    cases = dict(negative_n=(md, -1, 1, -1), negative_min=(md, n, -1, -1), over_span=(over, n, 1, -4),
                 **{k: (v, n, 1, -1) for k, v in bad.items()})
    for what, (x, n_, min_size, code) in cases.items():
        g, m, s = move(g0.copy()), move(m0.copy()), move(s0.copy())
        rc, n_peaks, n_labels = _raw(move(x), n_, min_size, g, m, s)
        assert rc == code and _lib.lib().asl_last_error(), what
        assert (n_peaks, n_labels) == (-5, -5), what
        assert _host(g).tobytes() == g0.tobytes() and _host(m).tobytes() == m0.tobytes(), what
        assert _host(s).tobytes() == s0.tobytes(), what
    with pytest.raises(_lib.AnnSoloMiError) as err:
        _lib.ssm_groups(move(bad['nan']), 1)
    assert err.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.AnnSoloMiError) as err:
        _lib.ssm_groups(move(over), 1)
    assert err.value.code == _lib.ERR_CAPACITY
    # n == 0: legal, nothing is written but the counts
    assert _raw(None, 0, 1, None) == (0, 0, 0)
    # the call after an error is a good call
    from ann_solo_amd import fdr
    assert _host(_lib.ssm_groups(move(md), 3)[0]).tobytes() == fdr.ssm_groups(md, 3).tobytes()


# ------------------------------------------------------------------------------------------ the scorers
def _profile_is_the_tables(scorer, groups, target, q, n):
    p = scorer.group_profile
    assert set(p) == {'group', 'mass', 'size', 'accepted'} and all(isinstance(c, np.ndarray) for c in p.values())
    assert p['group'][-1] == -1 and np.isnan(p['mass'][-1]) and np.isfinite(p['mass'][:-1]).all()
    assert (np.diff(p['group'][:-1]) > 0).all() and p['size'].sum() == n
    ids = np.unique(groups)
    assert p['group'][:-1].tolist() == ids[ids >= 0].tolist()
    hit = target & (q < scorer.fdr)
    for g, size, acc in zip(p['group'], p['size'], p['accepted']):
        assert size == (groups == g).sum() and acc == (hit & (groups == g)).sum(), g
    return p


def test_cosine_tdc_with_device_groups_is_cosine_tdc():
    from ann_solo_amd import fdr
    want = fdr.ssm_groups(TT._grouped_table().mass_diffs(), 40)
    ids, counts = np.unique(want, return_counts=True)
    assert ids[0] == -1 and len(ids) >= 4 and (counts[1:] >= 40).all()      # a residue and three groups
    ref = fdr.CosineTDC(40)
    b = TT._grouped_table()
    cos = b.score.copy()
    ref(b, 'open')
    for qvalues in (None, 'device'):
        dev = fdr.CosineTDC(40, qvalues=qvalues, device=DEV, groups='device', fdr=0.9)
        for _ in range(2):          # the same labels in every round
            a = TT._grouped_table()
            assert dev(a, 'open') is None
            assert a.q.tobytes() == b.q.tobytes() and a.score.tobytes() == b.score.tobytes()
            assert dev.n_groups == ref.n_groups == len(ids)
            p = _profile_is_the_tables(dev, want, ~a.is_decoy(), a.q, len(a))
            assert p['accepted'].sum() > 0 and len(p['group']) == len(ids)
            # the masses are the planted ones, to the bin
            for planted in (0.0, 15.9949, 79.9663):
                assert np.abs(p['mass'][:-1] - planted).min() < 0.02
        a.score = cos.copy()
        assert dev(a, 'std') is None and dev.group_profile is None          # a standard level has no groups


MODS = (0.0, 15.9949, 79.9663, -17.0265)


def _open_table():
    """The robust table of tests/fdr_cases.py as an open level: every query's precursor moved by one of four
    modification masses (row i by ``MODS[i % 4]``), so the level has four groups."""
    t = FC.robust_table()
    for i, meta in enumerate(t.query_meta[2]):
        meta['precursor_mz'] += MODS[i % 4] / 2
    return t


def _open_scorer_runs(make):
    """``make(groups, qvalues)`` on the robust table at the open level: without the switch, with it, with both."""
    out = []
    for groups, qvalues in ((None, None), ('device', None), ('device', 'device')):
        t = _open_table()
        s = make(groups, qvalues)
        assert s(t, 'open') is None and not s.fallback
        out.append((s, t))
    (ref, b) = out[0]
    labels = np.unique(fdr_groups(b, ref.min_group_size))
    assert len(labels) >= 3                                     # the level really is grouped
    for s, a in out[1:]:
        assert a.score.tobytes() == b.score.tobytes() and a.q.tobytes() == b.q.tobytes()
        assert s.n_groups == ref.n_groups == len(labels)
        assert len(s.trace) == len(ref.trace) == 3
        for x, y in zip(s.trace, ref.trace):
            assert x['grid'] == y['grid'] and all(p.tobytes() == r.tobytes() for p, r in zip(x['labels'], y['labels']))
        _profile_is_the_tables(s, fdr_groups(a, s.min_group_size), ~a.is_decoy(), a.q, len(a))
    assert ref.group_profile is None and (b.q <= 0.01).sum() > 500


def fdr_groups(table, min_group_size):
    from ann_solo_amd import fdr
    return fdr.ssm_groups(table.mass_diffs(), min_group_size)


def test_percolator_with_device_groups_is_percolator():
    from ann_solo_amd import fdr
    _open_scorer_runs(lambda g, q: fdr.PercolatorTDC(device=DEV, min_group_size=50, groups=g, qvalues=q))


def test_forest_with_device_groups_is_forest():
    from ann_solo_amd import fdr
    _open_scorer_runs(lambda g, q: fdr.ForestTDC(device=DEV, trees=16, min_group_size=50, groups=g, qvalues=q))


def test_a_span_over_the_cap_falls_back_to_the_host(caplog):
    """Nominals -32 768 and 32 768 in one level: ASL_ERR_CAPACITY, one warning, ``ssm_groups`` on the host -- the
    same q-values; a non-finite mass difference is a ValueError."""
    from ann_solo_amd import fdr

    def table(extreme):
        t = TT._grouped_table()
        meta = t.query_meta[2]
        for row, v in zip(range(4), extreme):       # (experimental - library precursor m/z) * charge
            meta[row]['precursor_mz'] = t.library_meta[2][int(t.lib_row[row])]['precursor_mz'] + v / 2
        return t
    wide = (-32768.0, 32768.0, -32768.001, 32768.001)
    a, b = table(wide), table(wide)
    assert np.rint(a.mass_diffs()).max() - np.rint(a.mass_diffs()).min() == 65536
    dev, ref = fdr.CosineTDC(40, qvalues='device', device=DEV, groups='device'), fdr.CosineTDC(40)
    with caplog.at_level(logging.WARNING):
        dev(a, 'open')
    ref(b, 'open')
    assert sum('span more than' in r.getMessage() for r in caplog.records) == 1
    assert a.q.tobytes() == b.q.tobytes() and dev.n_groups == ref.n_groups and dev.group_profile is None
    with pytest.raises(ValueError, match='non-finite'):
        dev(table((np.nan, 0.0, 0.0, 0.0)), 'open')


# ------------------------------------------------------------------------------------------ end to end
class _Recorder:
    """The engine's scorer, keeping the table of its last open call."""

    def __init__(self, scorer):
        self.scorer, self.open_call = scorer, None

    def __getattr__(self, name):
        return getattr(self.scorer, name)

    def __call__(self, table, mode):
        out = self.scorer(table, mode)
        if mode == 'open':
            self.open_call = (fdr_groups(table, self.scorer.min_group_size), ~table.is_decoy(), table.q.copy(),
                              len(table))
        return out


def test_the_switch_end_to_end(tmp_path):
    from ann_solo_amd import fdr
    from ann_solo_amd.config import Config
    from ann_solo_amd.library_store import pack_queries
    from ann_solo_amd.spectral_library import SpectralLibrary
    specs = TT._library()
    base = dict(num_list=8, num_probe=8, num_candidates=64, kmeans_niter=4, fragment_mz_tolerance=0.02,
                decoy_tolerance_unit='Da', seed=5, min_mz_range=100.0, device_decoys=True, fdr=0.05,
                fdr_min_group_size=20, precursor_tolerance_mass=20.0, precursor_tolerance_mode='ppm',
                device_fdr=True)
    tables = []
    for k, extra in enumerate((dict(), dict(device_groups=True, device_qvalues=True))):
        d = tmp_path / f'lib{k}'
        d.mkdir()
        eng = SpectralLibrary(FakeReader(specs, str(d / 'lib.splib')), config=Config.open_search(**base, **extra),
                              device=DEV)
        try:
            assert isinstance(eng._score_ssms, fdr.CosineTDC)
            assert eng._score_ssms.groups == ('device' if extra else None)
            eng._score_ssms = rec = _Recorder(eng._score_ssms)
            qs, qmeta = pack_queries(iter(TT._queries(specs)), eng.config, eng.device)
            tables.append(eng.search_packed(qs, qmeta, eng.library_meta))
            groups, target, q, n = rec.open_call
            if extra:
                assert n > 100 and rec.scorer.n_groups == len(np.unique(groups))
                p = _profile_is_the_tables(rec.scorer, groups, target, q, n)
                assert np.abs(p['mass'][:-1] - 15.9949).min() < 0.02       # the planted modification
            else:
                assert rec.scorer.group_profile is None
        finally:
            eng.shutdown()
    a, b = tables
    assert len(a) == len(b) > 100
    for name in ('charge', 'qrow', 'lib_row', 'open_level'):        # the accepted identifications
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)
    assert a.score.tobytes() == b.score.tobytes() and a.q.tobytes() == b.q.tobytes()
