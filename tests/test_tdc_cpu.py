"""The device q-values without a GPU: the numpy restatement tests/tdc_ref.py -- written from the C ABI's comment,
and what tests/test_gpu_tdc.py's cases are about -- equals the host code of ann_solo_amd/fdr.py
(``tdc_qvalues`` per group, ``_labels``) byte for byte on every case of tests/tdc_cases.py; the key map; the
switch, its errors, the parser and ``make_scorer``."""
import argparse
import os

import numpy as np
import pytest

import tdc_cases as TC
import tdc_ref as R
from ann_solo_amd import fdr
from ann_solo_amd.config import Config, add_arguments

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = [name for name, _ in TC.CASE_IDS]


def test_the_cases_hold_what_they_promise():
    assert TC.TILE >= 256 and TC.N_LEVELS > 256 * TC.TILE       # the counts' partials exceed one scan block
    seen = {(c[1], c[3]) for _, c in TC.CASE_IDS}
    assert seen >= {(s, g) for s in TC.SCORES for g in TC.GROUPS}
    assert {c[0] for _, c in TC.CASE_IDS} >= set(TC.SMALL_SIZES) | {TC.N_LEVELS, 300001}
    assert {c[2] for _, c in TC.CASE_IDS} == set(TC.TARGETS) and {c[4] for _, c in TC.CASE_IDS} == set(TC.USES)
    assert all((name[:-5] + '-desc' in NAMES) and (name[:-5] + '-asc' in NAMES) for name in NAMES if
               name.endswith('-desc'))
    z = TC.scores('zeros', 4096, np.random.default_rng(0))
    assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any() and (z < 0).any() and (z > 0).any()
    dn = TC.scores('denormal', 4096, np.random.default_rng(0)).view(np.uint64) & np.uint64((1 << 63) - 1)
    assert dn.max() == 40 and len(np.unique(dn)) == 41          # real denormals, not flushed to zero
    g = TC.groups('mixed', 257, np.random.default_rng(0))
    ids, counts = np.unique(g, return_counts=True)
    assert ids.min() == -1 and ids.max() == 5 and counts[ids == 4] == 1 and counts[ids == 5] == 2
    lo, hi = (TC.scores(k, 4096, np.random.default_rng(0)).view(np.uint64) for k in ('lowbyte', 'highbyte'))
    assert len(np.unique(lo >> np.uint64(8))) == 1 and len(np.unique(lo)) == 256
    assert len(np.unique(hi << np.uint64(8))) == 1 and len(np.unique(hi)) == 256 and np.isfinite(hi.view(float)).all()


@pytest.mark.parametrize('name', NAMES)
def test_restatement_equals_the_host_code(name):
    score, target, group, use, desc = TC.get(name)
    want = TC.host_q(name)
    with TC.ieee_denormals():
        assert R.tdc_qvalues(score, target, group, use, desc).tobytes() == want.tobytes()
        for level in (0.01, 0.5):
            q, lab = R.tdc_qvalues(score, target, group, use, desc, fdr=level)
            assert q.tobytes() == want.tobytes() and lab.dtype == np.int8
            assert lab.tobytes() == TC.host_labels(name, level).tobytes()
            if group is None:       # the scorers' own labelling, as it stands
                train = np.arange(len(score)) if use is None else np.nonzero(use)[0]
                own = fdr.PercolatorTDC(fdr=level, solver=(None, None))._labels(score, target, train, desc)
                assert own.tobytes() == lab.tobytes()


def test_the_key_map_is_strictly_monotone():
    with TC.ieee_denormals():
        _key_map_is_strictly_monotone()


def _key_map_is_strictly_monotone():
    tiny, tiny2 = np.array([1, 2], np.uint64).view(np.float64)      # (from the bit patterns: no arithmetic)
    big = np.finfo(np.float64).max
    s = np.array([-np.inf, -big, -1.0 - 2 ** -52, -1.0, -2.2250738585072014e-308, -tiny2, -tiny, 0.0, tiny,
                  tiny2, 2.2250738585072014e-308, 1.0, 1.0 + 2 ** -52, big, np.inf])
    assert (s.view(np.uint64)[5:7] == [(1 << 63) | 2, (1 << 63) | 1]).all() and (s[1:] > s[:-1]).all()
    up, down = R.score_key(s, False), R.score_key(s, True)
    assert up.dtype == np.uint64 and (up[1:] > up[:-1]).all() and (down[1:] < down[:-1]).all()
    for desc in (False, True):
        a, b = R.score_key(np.array([-0.0, 0.0]), desc)
        assert a == b
    g = np.array([np.iinfo(np.int32).min, -2, -1, 0, 1, np.iinfo(np.int32).max], np.int32)
    k = R.group_key(g)
    assert k.dtype == np.uint32 and (k[1:] > k[:-1]).all()


def test_restatement_refuses_what_the_entry_point_refuses():
    s, t = np.array([0.5, np.nan, 0.25]), np.array([True, False, True])
    with pytest.raises(ValueError, match='NaN'):
        R.tdc_qvalues(s, t)
    q = R.tdc_qvalues(s, t, use=np.array([1, 0, 1], np.uint8))      # a NaN in an unused row is legal
    assert np.isnan(q[1]) and q[0] == 0.5 and q[2] == 0.5      # (0 + 1) / 2 at the end, the minimum before it
    for bad in (np.nan, -0.5):
        with pytest.raises(ValueError, match='fdr'):
            R.tdc_qvalues(s[::2], t[::2], fdr=bad)
    with pytest.raises(ValueError, match='desc'):
        R.tdc_qvalues(s[::2], t[::2], desc=2)


# ------------------------------------------------------------------ the switch
def test_the_switch_and_its_errors():
    assert Config().device_qvalues is False
    p = argparse.ArgumentParser()
    add_arguments(p)
    assert p.parse_args([]).device_qvalues is False
    ns = p.parse_args(['--device_fdr', '--device_qvalues'])
    cfg = Config.from_reference(ns)
    assert cfg.device_qvalues is True and cfg.device_fdr is True
    with pytest.raises(ValueError, match='device_qvalues.*needs device_fdr'):
        Config(device_qvalues=True)
    with pytest.raises(ValueError, match='sharded'):
        Config(device_fdr=True, device_qvalues=True, num_gpus=2)
    assert Config(device_fdr=True, device_qvalues=True, num_gpus=1).device_qvalues


def test_make_scorer_hands_the_keyword_on():
    for kw, cls in ((dict(), fdr.CosineTDC), (dict(model='svm'), fdr.PercolatorTDC),
                    (dict(model='rf', device_forest=True), fdr.ForestTDC)):
        off = fdr.make_scorer(Config(device_fdr=True, **kw), device='cuda:0')
        on = fdr.make_scorer(Config(device_fdr=True, device_qvalues=True, **kw), device='cuda:0')
        assert isinstance(off, cls) and isinstance(on, cls)
        assert off.qvalues is None and on.qvalues == 'device' and on.device == 'cuda:0'
    with pytest.raises(ValueError, match='qvalues'):
        fdr.PercolatorTDC(qvalues='host')
    with pytest.raises(ValueError, match='qvalues'):
        fdr.CosineTDC(qvalues='gpu')


def test_no_hash_knows_the_switch():
    from ann_solo_amd.spectral_library import SpectralLibrary
    out = []
    for kw in (dict(device_fdr=True), dict(device_fdr=True, device_qvalues=True)):
        sl = SpectralLibrary.__new__(SpectralLibrary)
        sl.config = Config.open_search(**kw)
        out.append((sl._get_hyperparameter_hash(), sl._get_index_hash()))
    assert out[0] == out[1]


def test_entry_point_is_exported():
    from ann_solo_amd import _lib
    assert 'asl_tdc_qvalues' in _lib.EXPORTS and hasattr(_lib.lib(), 'asl_tdc_qvalues')
    assert _lib.TDC_TILE == TC.TILE
