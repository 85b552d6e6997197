"""Modification site localisation, host side: the numpy restatement (tests/localize_ref.py) on planted,
ambiguous and degenerate inputs, the configuration switch, the SSM columns and the wrapper's host checks."""
import argparse
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import localize_cases as LC     # noqa: E402
import localize_ref as R        # noqa: E402

TOL = 0.02


@functools.lru_cache(maxsize=None)
def planted(n=300, seed=20261):
    """``n`` planted cases from a fixed seed with their reference results: peptides of 6 .. 30 residues,
    one of the five masses on a random residue, a complete singly charged ladder."""
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        L = int(rng.integers(6, 31))
        cases.append(LC.planted_case(rng, L, LC.DELTAS[i % len(LC.DELTAS)], int(rng.integers(0, L))))
    return cases, LC.reference(cases, TOL, 'Da')


def test_planted_sites():
    """Of 300 cases those are kept for which the restatement names the planted site and no other (a chance
    match of a doubly charged fragment can tie or beat a neighbouring site): at least 100, in fact nearly
    all; every kept case has a positive margin and gains over the unmodified peptide."""
    cases, refs = planted()
    kept = [(c, r) for c, r in zip(cases, refs) if r['best_lo'] == r['best_hi'] == c['site']]
    print('planted cases kept: %d of %d' % (len(kept), len(cases)))
    assert len(kept) >= 100
    for c, r in kept:
        assert r['best_lo'] == r['best_hi'] == c['site'] and r['n_best'] == 1
        assert r['best_score'] > r['runner_score'] and r['best_score'] > r['none_score']
        assert r['best_count'] >= 2 * (c['L'] - 1)            # the whole ladder is found
        assert r['best_score'] == r['site_score'][c['site']]


def test_ambiguous_sites():
    """Without b_{j+1} and y_{L-j-1} (plain or shifted: the spectrum has neither) nothing tells site j from
    j + 1: both add the same addends in the same order, and tie bit for bit."""
    rng = np.random.default_rng(7)
    n = 0
    for i in range(40):
        L = int(rng.integers(6, 31))
        j = int(rng.integers(0, L - 1))
        c = LC.planted_case(rng, L, LC.DELTAS[i % 5], j, drop_b=(j + 1,), drop_y=(L - j - 1,))
        r = R.localize_ref(c['mz'], c['intensity'], c['masses'], 0.0, 0.0, 2, c['delta'], TOL, 'Da')
        # the dropped pair is absent under both hypotheses, chance matches apart
        if not (r['pick'][0, j + 1] < 0).all() or not (r['pick'][1, L - j - 1] < 0).all():
            continue
        n += 1
        assert (r['best_lo'], r['best_hi'], r['n_best']) == (j, j + 1, 2), (i, j, r['site_score'])
        assert LC.bits(r['site_score'][j:j + 1])[0] == LC.bits(r['site_score'][j + 1:j + 2])[0]
    assert n >= 30


def test_degenerate_inputs():
    rng = np.random.default_rng(3)
    pep = LC.parse('ACDEFGHIK')
    L = 9
    # no peaks: every score 0, every site ties
    r = R.localize_ref([], [], pep.masses, 0.0, 0.0, 2, 15.994915, TOL, 'Da')
    assert (r['best_lo'], r['best_hi'], r['n_best'], r['best_count']) == (0, L - 1, L, 0)
    assert r['best_score'] == r['runner_score'] == r['none_score'] == 0.0 and not r['site_score'].any()
    # delta = 0: plain and shifted fragments coincide, every site ties with the unmodified peptide
    c = LC.planted_case(rng, 14, 0.0, 5)
    r = R.localize_ref(c['mz'], c['intensity'], c['masses'], 0.0, 0.0, 2, 0.0, TOL, 'Da')
    assert (r['best_lo'], r['best_hi'], r['n_best']) == (0, 13, 14)
    assert r['best_score'] == r['runner_score'] == r['none_score'] > 0.0
    assert len(set(LC.bits(r['site_score']).tolist())) == 1
    # L = 2: one b and one y fragment; the mass on residue 0 shifts b_1, on residue 1 y_1
    m = LC.parse('AK').masses
    for site in (0, 1):
        b, y = LC.ladder_mz(m, site, 79.966331)
        r = R.localize_ref(np.sort(np.float32([b[0], y[0]])), [1.0, 1.0], m, 0.0, 0.0, 1, 79.966331, TOL, 'Da')
        assert (r['best_lo'], r['best_hi'], r['best_count']) == (site, site, 2)
        assert r['best_score'] == 2.0 and r['runner_score'] == 0.0 and r['none_score'] == 1.0
    # equal intensities inside one window: the lowest index wins; a larger one further on wins over both
    b, _ = LC.ladder_mz(pep.masses, 0, 0.0)
    x = np.float32(b[2])
    mz = np.float32([x - 0.01, x, x + 0.01])
    r = R.localize_ref(mz, [2.0, 2.0, 2.0], pep.masses, 0.0, 0.0, 1, 100.0, TOL, 'Da')
    assert r['pick'][0, 3, 0, 0] == 0 and r['none_score'] == 2.0
    r = R.localize_ref(mz, [2.0, 2.0, 3.0], pep.masses, 0.0, 0.0, 1, 100.0, TOL, 'Da')
    assert r['pick'][0, 3, 0, 0] == 2 and r['none_score'] == 3.0


def test_config_flag_and_hashes():
    from ann_solo_amd.config import Config, add_arguments
    from ann_solo_amd.library_store import store_hash
    from ann_solo_amd.spectral_library import SpectralLibrary
    p = argparse.ArgumentParser()
    add_arguments(p)
    assert p.parse_args([]).localize_modifications is False
    cfg = Config.from_reference(p.parse_args(['--localize_modifications']))
    assert cfg.localize_modifications is True and Config().localize_modifications is False
    with pytest.raises(ValueError, match='localize_modifications'):
        Config(localize_modifications=True, num_gpus=2)
    Config(localize_modifications=True, num_gpus=1)

    def hashes(cfg):
        sl = SpectralLibrary.__new__(SpectralLibrary)
        sl.config = cfg
        return sl._get_hyperparameter_hash(), sl._get_index_hash(), store_hash(cfg, 'abc', 'peaks')
    for kw in ({}, dict(index='ivfpq'), dict(precursor_tolerance_mass_open=300.0, precursor_tolerance_mode_open='Da')):
        assert hashes(Config(**kw)) == hashes(Config(localize_modifications=True, **kw))


def test_ssm_table_columns():
    from ann_solo_amd.spectral_library import BatchResult, SSMTable
    qmeta = {2: [dict(identifier=f'q{i}', index=i, precursor_charge=2, precursor_mz=500.0 + i) for i in range(4)]}
    lmeta = {2: [dict(identifier=f'l{i}', peptide='PEPTIDEK', precursor_mz=480.0 + i) for i in range(4)]}

    def table(rows):
        t = SSMTable(qmeta, lmeta)
        res = BatchResult(np.asarray(rows, np.int32), np.ones(len(rows)), np.ones(len(rows), np.int32),
                          np.zeros(len(rows), np.int32), np.zeros((len(rows), 1, 2), np.uint32))
        t.add_batch(2, np.arange(len(rows)), np.asarray(rows), np.ones(len(rows)), res)
        return t
    t = table([0, -1, 2, 3])
    assert len(t) == 3
    assert t.open_level.dtype == bool and not t.open_level.any()
    assert t.mod_mass.dtype == np.float64 and np.isnan(t.mod_mass).all()
    assert t.mod_site_lo.dtype == t.mod_site_hi.dtype == np.int32
    assert (t.mod_site_lo == -1).all() and (t.mod_site_hi == -1).all()
    for k in ('mod_site_score', 'mod_site_margin', 'mod_site_gain'):
        assert getattr(t, k).dtype == np.float64 and np.isnan(getattr(t, k)).all()
    s = t[1]
    assert np.isnan(s.mod_mass) and s.mod_site_lo == s.mod_site_hi == -1 and np.isnan(s.mod_site_gain)
    t.open_level[:] = [False, True, True]
    t.mod_mass[1], t.mod_site_lo[1], t.mod_site_hi[1] = 15.994915, 3, 4
    t.mod_site_score[1], t.mod_site_margin[1], t.mod_site_gain[1] = 7.5, 0.25, 2.0
    s = t[1]
    assert (s.mod_mass, s.mod_site_lo, s.mod_site_hi) == (15.994915, 3, 4)
    assert (s.mod_site_score, s.mod_site_margin, s.mod_site_gain) == (7.5, 0.25, 2.0)
    u = t.take([1, 0])
    assert u.open_level.tolist() == [True, False] and u.mod_site_lo.tolist() == [3, -1]
    assert u.mod_site_score[0] == 7.5 and np.isnan(u.mod_site_score[1])
    w = SSMTable.concat([table([1]), t, u])
    assert len(w) == 6 and w.open_level.tolist() == [False, False, True, True, True, False]
    assert w.mod_site_hi.tolist() == [-1, -1, 4, -1, 4, -1]
    assert w.mod_site_margin[2] == 0.25 and w.mod_site_gain[4] == 2.0 and np.isnan(w.mod_mass[0])
    uid = {2: np.asarray([0, 1, 2, 2])}
    f = t.first_per_uid(uid)
    assert len(f) == 2 and f.mod_site_lo.tolist() == [-1, 3]


def _two_cases():
    rng = np.random.default_rng(1)
    return [LC.planted_case(rng, 8, 15.994915, 2), LC.planted_case(rng, 11, 79.966331, 9)]


def test_wrapper_refuses_mismatched_lengths():
    from ann_solo_amd import localize as lz
    q, seq, mass, nterm, cterm, zmax, delta = LC.pack_cases(_two_cases())
    for bad in ((q, seq[:-1], mass, nterm, cterm, zmax, delta), (q, seq, mass[:-1], nterm, cterm, zmax, delta),
                (q, seq, mass, nterm[:1], cterm, zmax, delta), (q, seq, mass, nterm, np.zeros(3), zmax, delta),
                (q, seq, mass, nterm, cterm, zmax[:1], delta), (q, seq, mass, nterm, cterm, zmax, delta[:1])):
        with pytest.raises(ValueError, match='lengths'):
            lz.localize_batch(*bad, TOL, 'Da', 'cpu')
    with pytest.raises(ValueError, match='unit'):
        lz.localize_batch(q, seq, mass, nterm, cterm, zmax, delta, TOL, 'mmu', 'cpu')
    with pytest.raises(ValueError, match='peptides'):
        lz.localize_peptides(q, ['PEPTIDEK'], delta, TOL, 'Da', 'cpu')
    with pytest.raises(ValueError, match='Nope'):
        lz.localize_peptides(q, ['PEPTIDEK', 'PEPT[Nope]IDEK'], delta, TOL, 'Da', 'cpu')


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU behaviour')
def test_no_cpu_fallback():
    from ann_solo_amd import _lib
    from ann_solo_amd import localize as lz
    with pytest.raises(_lib.AnnSoloMiError, match='no HIP device'):
        lz.localize_batch(*LC.pack_cases(_two_cases()), TOL, 'Da', 'cpu')


def test_symbol_is_exported():
    from ann_solo_amd import _lib
    assert 'asl_localize_batch' in _lib.EXPORTS
    assert hasattr(_lib.lib(), 'asl_localize_batch')
