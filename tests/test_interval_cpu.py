"""Per-query precursor intervals (ASL_TOL_INTERVAL), the parts that need no GPU: the reference of
tests/interval_ref.py (the oracle's Da test over a key column masked per query) equals the direct definition
lo <= key <= hi, the inputs of the GPU tests have the properties those tests rely on, the ``Config`` / flag
validation, and the host derivation of the open level's intervals."""
import argparse
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import interval_ref as R
from ann_solo_amd.config import Config, add_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, NPROBE, NLIST, NQ, COPIES = 256, 8, 16, 48, 8


# ------------------------------------------------------------------ the construction is the definition
def _scalar_rule(key, lo, hi):
    """The rule of include/annsolo_mi.h, one Python float comparison at a time."""
    return np.array([bool(lo <= float(v) and float(v) <= hi) for v in np.asarray(key, np.float32)], bool)


def test_masked_key_construction_is_the_direct_definition(O):
    rng = np.random.default_rng(11)
    key = rng.uniform(300.0, 1500.0, 400).astype(np.float32)
    key[::9] = np.nan
    key[5], key[6] = np.float32(np.inf), np.float32(-np.inf)
    k64 = key.astype(np.float64)
    a, b = float(k64[10]), float(k64[200])
    lo_, hi_ = min(a, b), max(a, b)
    bounds = [(lo_, hi_),                                             # keys equal to a bound
              (np.nextafter(lo_, np.inf), np.nextafter(hi_, -np.inf)),  # bounds just inside the two keys
              (np.nextafter(lo_, -np.inf), np.nextafter(hi_, np.inf)),  # ... and just outside
              (a, a), (np.nextafter(a, np.inf), np.nextafter(a, np.inf)), (np.nextafter(a, -np.inf), a),
              (hi_, lo_),                                             # lo > hi: empty
              (np.nan, hi_), (lo_, np.nan), (np.nan, np.nan),
              (-np.inf, np.inf), (-np.inf, lo_), (hi_, np.inf), (np.inf, np.inf), (np.inf, -np.inf)]
    bounds += [tuple(sorted(rng.uniform(250.0, 1550.0, 2))) for _ in range(12)]
    counts = []
    for lo, hi in bounds:
        want = _scalar_rule(key, lo, hi)
        assert np.array_equal(R.interval_mask(key, lo, hi), want), (lo, hi)
        key_i = R.masked_key(key, lo, hi)
        assert key_i.dtype == np.float32
        assert np.array_equal(np.isfinite(key_i) | np.isinf(key_i), want), (lo, hi)
        assert np.array_equal(key_i[want].view(np.uint32), key[want].view(np.uint32))
        finite = want & np.isfinite(key)           # (an infinite key passes the rule only under an infinite bound;
        got = R.oracle_passes(O, np.where(finite, key_i, np.float32(np.nan)))   # the oracle's |q - l| is then inf)
        assert np.array_equal(got, finite), (lo, hi)
        counts.append(int(want.sum()))
    assert counts[0] == counts[1] + 2 == counts[2] and counts[3] == 1 and counts[4] == 0 and counts[5] == 1
    assert counts[6] == counts[7] == counts[8] == counts[9] == 0
    assert counts[10] == int((~np.isnan(key)).sum())
    assert not R.interval_mask(np.float32([np.nan]), -np.inf, np.inf)[0]


def test_header_and_bindings_name_the_mode():
    from ann_solo_amd import _lib, faiss_compat
    head = open(os.path.join(ROOT, 'include', 'annsolo_mi.h')).read()
    assert re.search(r'#define\s+ASL_TOL_INTERVAL\s+2\b', head)
    assert re.search(r'const double \*precursor_window;\s*\} asl_search_params_t;', head)
    assert faiss_compat.TOL_MODES == {'Da': 0, 'ppm': 1, 'interval': 2}
    names = [f[0] for f in _lib.AslSearchParams._fields_]
    assert names[-1] == 'precursor_window' and names[-2] == 'use_ann'
    P = _lib.AslSearchParams(10.96, 0.04, 42, 256, 8, 2, 300.0, 0, 0.02, 1, 1)
    assert P.precursor_window is None                                   # NULL unless given
    assert _lib.AslSearchParams.precursor_window.offset % C.sizeof(C.c_void_p) == 0
    with pytest.raises(ValueError):
        faiss_compat._window_operand(np.zeros(5), 5, 'interval', 't')   # [nq] where [nq, 2] is needed
    assert faiss_compat._window_operand(np.zeros(5, np.float32), 5, 'Da', 't').dtype == np.float64
    with pytest.raises(KeyError):
        faiss_compat._window_operand(np.zeros(5), 5, 'mDa', 't')
    w = faiss_compat._window_operand(np.zeros((5, 2), np.float32), 5, 'interval', 't')
    assert w.dtype == np.float64 and w.flags['C_CONTIGUOUS']


# ------------------------------------------------------------------ Config, flags
def test_config_and_flags():
    assert Config().precursor_window_open is None and Config.open_search().precursor_window_open is None
    cfg = Config.open_search(precursor_window_open=(-150, 500))
    assert cfg.precursor_window_open == (-150.0, 500.0)
    assert Config.open_search(precursor_window_open=[7.5, 7.5]).precursor_window_open == (7.5, 7.5)
    for bad in ((500, -150), (np.nan, 1.0), (1.0,), 'wide', (1, 2, 3)):
        with pytest.raises(ValueError):
            Config.open_search(precursor_window_open=bad)
    with pytest.raises(ValueError, match='precursor_tolerance_mass_open'):
        Config(precursor_window_open=(-150, 500))                       # the cascade switch is off
    with pytest.raises(ValueError, match='num_gpus'):
        Config.open_search(precursor_window_open=(-150, 500), num_gpus=2)
    Config.open_search(precursor_window_open=(-150, 500), num_gpus=1)
    p = argparse.ArgumentParser()
    p.add_argument('--precursor_tolerance_mass_open', type=float, default=None)
    p.add_argument('--precursor_tolerance_mode_open', type=str, default=None)
    add_arguments(p)
    ns = p.parse_args([])
    assert ns.precursor_window_open_low is None and ns.precursor_window_open_high is None
    assert Config.from_reference(ns).precursor_window_open is None
    opened = ['--precursor_tolerance_mass_open', '500', '--precursor_tolerance_mode_open', 'Da']
    ns = p.parse_args(opened + ['--precursor_window_open_low', '-150', '--precursor_window_open_high', '500'])
    assert Config.from_reference(ns).precursor_window_open == (-150.0, 500.0)
    for one in ('low', 'high'):                                         # both or neither
        with pytest.raises(ValueError, match='go together'):
            Config.from_reference(p.parse_args(opened + [f'--precursor_window_open_{one}', '10']))
    with pytest.raises(ValueError):                                     # needs the open level
        Config.from_reference(p.parse_args(['--precursor_window_open_low', '-150', '--precursor_window_open_high',
                                            '500']))
    with pytest.raises(ValueError):
        Config.from_reference(p.parse_args(opened + ['--precursor_window_open_low', '5',
                                                     '--precursor_window_open_high', '-5']))
    with pytest.raises(SystemExit):
        p.parse_args(['--precursor_window_open_low', 'wide'])


# ------------------------------------------------------------------ the host derivation
def test_open_level_intervals_from_the_signed_range():
    from ann_solo_amd.spectral_library import open_window_intervals, isolation_windows
    rng = np.random.default_rng(3)
    q = rng.uniform(300.0, 1500.0, 64)
    for z, (lo_da, hi_da) in ((2, (-150.0, 500.0)), (3, (-50.0, 250.0)), (2, (10.0, 250.0)), (1, (-250.0, -10.0))):
        w = open_window_intervals(q, z, (lo_da, hi_da))
        assert w.dtype == np.float64 and w.shape == (64, 2)
        assert np.array_equal(w[:, 0], q - hi_da / z) and np.array_equal(w[:, 1], q - lo_da / z)
        assert np.array_equal(w, R.derived(q, z, lo_da, hi_da)) and (w[:, 0] <= w[:, 1]).all()
    # dyadic values: (q - l) * z, q - hi_da / z and q - lo_da / z are all exact, so the interval test IS the
    # test on the mass difference -- at the bounds too
    qd = np.arange(600.0, 632.0, 0.5)
    lib = np.arange(300.0, 900.0, 0.25).astype(np.float32)
    w = open_window_intervals(qd, 2, (-150.0, 500.0))
    for i in range(len(qd)):
        md = (qd[i] - lib.astype(np.float64)) * 2.0
        assert np.array_equal(R.interval_mask(lib, w[i, 0], w[i, 1]), (md >= -150.0) & (md <= 500.0)), i
    assert R.interval_mask(lib, w[0, 0], w[0, 1])[[np.argmax(lib == 350.0), np.argmax(lib == 675.0)]].all()
    # isolation windows of the queries' metadata: all or nothing
    meta = [{'identifier': i, 'isolation_window': (400.0 + i, 404.0 + i)} for i in range(5)]
    assert np.array_equal(isolation_windows(meta, 5), np.array([[400.0 + i, 404.0 + i] for i in range(5)]))
    meta[3] = {'identifier': 3}
    assert isolation_windows(meta, 5) is None
    assert isolation_windows(None, 5) is None and isolation_windows([], 0) is None
    for bad in ((404.0, 400.0), (400.0,), (400.0, np.nan), 400.0, (1.0, 2.0, 3.0)):       # no pair lo <= hi
        meta[3] = {'identifier': 3, 'isolation_window': bad}
        with pytest.raises(ValueError, match='isolation_window'):
            isolation_windows(meta, 5)


def test_open_level_windows_of_the_cascade():
    from ann_solo_amd.spectral_library import SpectralLibrary
    q_pmz = np.array([500.25, 612.5, 733.125])
    qs = SimpleNamespace(n=3, precursor_mz=q_pmz)
    sl = SpectralLibrary.__new__(SpectralLibrary)
    sl._dist = None
    sl.config = Config.open_search()
    plain = {2: [{'identifier': i} for i in range(3)]}
    assert sl._open_level_windows(qs, plain, 2) is None                  # the symmetric window, as ever
    sl.config = Config.open_search(precursor_window_open=(-150, 500))
    assert np.array_equal(sl._open_level_windows(qs, plain, 2), R.derived(q_pmz, 2, -150.0, 500.0))
    iso = {2: [{'identifier': i, 'isolation_window': (q_pmz[i] - 1.0, q_pmz[i] + 3.0)} for i in range(3)]}
    want = np.stack([q_pmz - 1.0, q_pmz + 3.0], 1)
    assert np.array_equal(sl._open_level_windows(qs, iso, 2), want)      # instead of the derived ones
    sl.config = Config.open_search()
    assert np.array_equal(sl._open_level_windows(qs, iso, 2), want)
    sl._dist = SimpleNamespace(world=2)
    sl.config = Config.open_search()
    assert sl._open_level_windows(qs, plain, 2) is None
    with pytest.raises(ValueError, match='isolation windows.*sharded'):   # never silently the symmetric window
        sl._open_level_windows(qs, iso, 2)
    sl.config = Config.open_search(precursor_window_open=(-150, 500))
    sl.config.num_gpus = 0
    with pytest.raises(ValueError, match='sharded'):
        sl._open_level_windows(qs, plain, 2)
    with pytest.raises(ValueError, match='sharded'):
        sl._search_batch(SimpleNamespace(n=3), 2, 'open', windows=want)


# ------------------------------------------------------------------ the inputs of the GPU tests
@pytest.fixture(scope='module')
def world(O):
    lib0, aux, lib = R.tie_library()
    q = R.tie_queries(lib0, aux, NQ, seed=72, with_copies=COPIES)
    xb, xq = R.encode(O, lib), R.encode(O, q)
    cen = O.kmeans(xb, NLIST, niter=4, seed=1234)
    ivf = O.HostIVF(cen, O.assign(xb, cen), xb)
    key = np.asarray(lib.numpy()[4], np.float64).astype(np.float32)
    q_pmz = q.numpy()[4].astype(np.float64)
    wins, one_rows = R.window_cases(q_pmz, key, COPIES)
    return ivf, xq, key, q_pmz, wins, one_rows


def test_conditions_the_gpu_tests_rely_on(O, world):
    ivf, xq, key, q_pmz, wins, one_rows = world
    D0, I0 = ivf.search(xq, K, NPROBE)
    sym = R.derived(q_pmz, 2, -250.0, 250.0)

    def post(w):        # the candidates of the 'post' order: the plain row's ids that pass
        return [set(I0[i][I0[i] >= 0][R.interval_mask(key[I0[i][I0[i] >= 0]], w[i, 0], w[i, 1])].tolist())
                for i in range(NQ)]
    a, b = post(wins['m50_p250']), post(sym)
    assert sum(x != y for x, y in zip(a, b)) >= NQ // 2                  # the asymmetric window changes the sets
    assert all(x <= y for x, y in zip(a, b))
    # 'pre' order: short rows (a window with fewer than k vectors in the probed lists) ...
    _, I = R.index_rows(O, ivf, xq, K, NPROBE, key, wins['m50_p250'])
    assert 0 < int((I < 0).any(1).sum())
    assert (I[:, 0] >= 0).any()
    # ... and rows cut by ties at the k-th score: the copies of row 0 score alike, more of them than k = 64
    D65, I65 = R.index_rows(O, ivf, xq[:COPIES], 65, NPROBE, key, wins['m50_p250'][:COPIES])
    assert (I65 >= 0).all() and (I65 < 400).all()
    assert (D65[:, 63].view(np.uint32) == D65[:, 64].view(np.uint32)).all()
    # the unmodified match: inside (-50, +250), outside (+10, +250) and (-250, -10)
    same = np.float32(q_pmz[COPIES:]).astype(np.float64)                 # a row at the query's own m/z
    for name, inside in (('m50_p250', True), ('p10_p250', False), ('m250_m10', False), ('iso4', True)):
        w = wins[name][COPIES:]
        got = np.array([R.interval_mask(np.float32([same[i]]), w[i, 0], w[i, 1])[0] for i in range(len(same))])
        assert (got == inside).all(), name
    # empty windows: lo > hi, a NaN bound; exactly one row; every row
    for i in range(NQ):
        assert not R.interval_mask(key, *wins['empty'][i]).any()
        m = R.interval_mask(key, *wins['one_row'][i])
        assert m.sum() == 1 and m[one_rows[i]]
        assert R.interval_mask(key, *wins['all'][i]).all()
        nan = np.isnan(wins['nan_some'][i]).any()
        assert nan == (i % 5 == 0 or i % 7 == 3)
        assert R.interval_mask(key, *wins['nan_some'][i]).any() != nan
    assert 0 < sum(np.isnan(wins['nan_some']).any(1)) < NQ
    w = wins['iso4']
    assert np.allclose(w[:, 1] - w[:, 0], 4.0) and not np.allclose((w[:, 0] + w[:, 1]) / 2, q_pmz)
    # (-inf, +inf) is the Da mode with tol = 1e9; the dyadic case is the Da mode at tol 256
    for i in range(0, NQ, 7):
        assert np.array_equal(R.interval_mask(key, -np.inf, np.inf),
                              [O.precursor_ok(q_pmz[i], v, 2, 1e9, 'Da') for v in key])
    qd = np.round(q_pmz * 2.0) / 2.0
    for i in range(0, NQ, 5):
        assert np.array_equal(R.interval_mask(key, qd[i] - 128.0, qd[i] + 128.0),
                              [O.precursor_ok(qd[i], v, 2, 256.0, 'Da') for v in key])
