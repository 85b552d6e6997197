"""Chimeric search, host side: the numpy restatement of the depletion (tests/deplete_ref.py) on its
properties and against the oracle's dot product, the configuration switch, and the residue level of the
engine on the oracle backend with ``chimeric.deplete_batch`` answered by the restatement."""
import argparse
import logging

import numpy as np
import pytest

import deplete_cases as DC
import deplete_ref as R
import ppm_ref
from ann_solo_amd.config import Config, add_arguments

TOL = 0.02
SHIFT, PPM = R.SCORE_SHIFT, R.SCORE_FRAGMENT_PPM


def _one(q_mz, q_int, q_pmz, l_mz, l_chg, l_pmz, z, tol=TOL, flags=0, min_peaks=1, min_range=0.0):
    return R.deplete_one(np.asarray(q_mz, np.float32), np.asarray(q_int, np.float32), q_pmz,
                         np.asarray(l_mz, np.float32), None if l_chg is None else np.asarray(l_chg, np.uint8), l_pmz, z,
                         tol, flags, min_peaks, min_range)


# ------------------------------------------------------------------ the reference's own properties
def test_fmaf_is_a_true_fused_multiply_add():
    """One rounding per step: a case where float32(a * a + acc) rounded through double differs, and the two
    implementations (libm, the exact two-step) against each other on random operands."""
    a, c = np.float32(1.0 + 2.0 ** -12), np.float32(-1.0)
    exact = float(a) * float(a) + float(c)                  # 2^-11 + 2^-24: exact in double
    assert R.fmaf(a, a, c) == np.float32(exact)
    assert np.float32(a * a) + c != np.float32(exact)       # (the unfused float32 chain loses the 2^-24)
    libm, own = R._libm_fmaf(), R._exact_fmaf()
    if libm is None or own is None:         # (one implementation only on this machine: nothing to compare)
        return
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 6, 4000)).astype(np.float32)
    y = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 6, 4000)).astype(np.float32)
    # sums that cancel: where a second rounding would show
    z = (-(x.astype(np.float64) * y.astype(np.float64))).astype(np.float32)
    for a, b, c in zip(x, y, np.where(rng.random(4000) < 0.5, z, x[::-1])):
        assert libm(a, b, c).tobytes() == own(a, b, c).tobytes(), (a, b, c)


def test_nothing_explained_gives_the_input_back_renormalised():
    rng = np.random.default_rng(1)
    q_mz = np.sort(rng.uniform(200, 1400, 40)).astype(np.float32)
    q_int = rng.uniform(0.1, 1.0, 40).astype(np.float32)
    one = _one(q_mz, q_int, 600.0, [50.0, 60.0], [1, 0], 600.0, 2, min_peaks=10, min_range=250.0)
    assert one['count'] == 40 and one['valid'] and np.array_equal(one['src'], np.arange(40))
    assert np.array_equal(one['mz'], q_mz)
    acc = np.float32(0.0)
    for v in q_int:
        acc = R.fmaf(v, v, acc)
    assert one['energy'] == acc and np.array_equal(one['intensity'], q_int / np.sqrt(acc, dtype=np.float32))
    # a unit-norm query: the kept energy is 1 up to the rounding of its own normalisation
    unit = one['intensity']
    again = _one(q_mz, unit, 600.0, [50.0], [0], 600.0, 2)
    assert abs(float(again['energy']) - 1.0) < 40 * 2.0 ** -23


def test_everything_explained_gives_count_0_invalid():
    l_mz = np.arange(20, dtype=np.float32) * 50 + 200
    one = _one(l_mz + np.float32(0.01), np.ones(20), 600.0, l_mz, np.zeros(20), 600.0, 2, min_peaks=0)
    assert one['count'] == 0 and not one['valid'] and one['energy'] == 0 and len(one['src']) == 0


def test_gate_closed_means_only_c_0():
    """The query holds a peak on a library peak and one on its c = 1 shifted position: with the gate closed
    (|pmd| below the tolerance, or the flag clear) only the first is explained."""
    l_mz, z = [500.0], 2
    for flags, tol in ((SHIFT, 0.02), (SHIFT | PPM, 20.0)):
        closed, opened = DC.gate_precursors(700.0, z, tol, flags)
        for q_pmz, is_open in ((closed, False), (opened, True), (700.0 + 8.0, True)):
            pmd = (q_pmz - 700.0) * z
            q_mz = np.sort(np.asarray([500.0, 500.0 + pmd, 900.0], np.float32))
            assert (R.shifts_of(q_pmz, 700.0, z, tol, flags)[0] == z + 1) == is_open
            if q_pmz == 708.0:
                on = _one(q_mz, [1, 1, 1], q_pmz, l_mz, [0], 700.0, z, tol, flags)
                off = _one(q_mz, [1, 1, 1], q_pmz, l_mz, [0], 700.0, z, tol, flags & ~SHIFT)
                assert list(on['src']) == [2] and list(off['src']) == [1, 2]      # 516 is the c = 1 position


def test_an_annotated_library_peak_shifts_only_by_its_own_charge():
    z, l_pmz, q_pmz = 3, 600.0, 604.0           # pmd = 12: shifts 12, 6, 4
    q_mz = [512.0, 506.0, 504.0]
    for chg, kept in ((0, []), (1, [1, 2]), (2, [0, 2]), (3, [0, 1])):
        one = _one(q_mz[::-1], [1, 1, 1], q_pmz, [500.0], [chg], l_pmz, z, flags=SHIFT)
        assert sorted(q_mz[::-1][i] for i in one['src']) == sorted(q_mz[i] for i in kept), chg
    none = _one(q_mz[::-1], [1, 1, 1], q_pmz, [500.0], None, l_pmz, z, flags=SHIFT)      # charge == NULL: all 0
    assert none['count'] == 0
    # a charge that makes no shifts at all: z + 1 <= 0 leaves even c = 0 out, as in the rescoring's loop
    assert _one([500.0], [1], q_pmz, [500.0], [0], l_pmz, -1, flags=SHIFT)['count'] == 1


def test_skip_rule_padding_and_errors():
    ssms = [DC.make_ssm(np.random.default_rng(i), qn, 20, 2, 15.994915, SHIFT) for i, qn in enumerate((5, 0, 12, 7))]
    q, lib, rows = DC.pack(ssms, skip=(2,))
    out = R.deplete_batch(q, lib, rows, TOL, SHIFT, 3, 10.0)
    assert out['mz'].shape == (4, 12) and out['count'][2] == 0 and out['valid'][2] == 0 and out['kept_energy'][2] == 0
    assert not out['mz'][2].any() and not out['intensity'][2].any() and not out['src'][2].any()
    assert out['count'][1] == 0 and out['valid'][1] == 0
    for s in range(4):
        k = out['count'][s]
        assert not out['mz'][s, k:].any() and not out['intensity'][s, k:].any() and not out['src'][s, k:].any()
    with pytest.raises(OverflowError):
        R.deplete_batch(q, lib, rows, TOL, SHIFT, 3, 10.0, stride=11)
    for bad in (dict(tol=-1.0), dict(tol=float('nan')), dict(flags=4)):
        with pytest.raises(ValueError):
            R.deplete_batch(q, lib, rows, bad.get('tol', TOL), bad.get('flags', SHIFT), 3, 10.0)
    with pytest.raises(ValueError):
        R.deplete_batch(q, lib, np.array([0, 1, 2, 4]), TOL, SHIFT, 3, 10.0)


def test_validity_edges():
    mz = np.array([100.0, 200.0, 300.0, 350.0], np.float32)
    above = float(np.nextafter(np.float32(250.0), np.float32(1e9)))
    for min_peaks, min_range, want in ((4, 250.0, True), (5, 250.0, False), (4, above, False)):
        one = _one(mz, np.ones(4), 500.0, [50.0], [0], 500.0, 2, min_peaks=min_peaks, min_range=min_range)
        assert one['valid'] == want, (min_peaks, min_range)


# ------------------------------------------------------------------ superset of the dot product's matches
@pytest.mark.parametrize('unit', ('Da', 'ppm'))
@pytest.mark.parametrize('shift', (False, True))
def test_the_winners_matched_peaks_never_survive(O, unit, shift):
    """Every query peak in the peak matches of the single-candidate dot product is explained. Da: the oracle's
    ``orc_dot_pair``; ppm, which the oracle's dot product does not have: tests/ppm_ref.py, the restatement the
    ppm mode is held against (test_ppm_cpu.py holds it against the oracle at Da)."""
    flags = R.flags_of(shift, unit)
    tol = DC.tol_of(flags)
    rng = np.random.default_rng(11 + 2 * shift + (unit == 'ppm'))
    n_pairs = n_kept = 0
    for t in range(60):
        z = (1, 2, 3, 5)[t % 4]
        s = DC.make_ssm(rng, int(rng.integers(1, 80)), int(rng.integers(1, 60)), z, DC.PMD_KINDS[t % 6], flags,
                        'none' if t % 5 == 0 else 'mixed')
        if unit == 'Da':
            _, m = O.dot_pair(s['q_mz'], s['q_int'], s['q_pmz'], s['l_mz'], s['l_int'], s['l_chg'], s['l_pmz'], z, tol,
                              shift)
        else:
            _, m = ppm_ref.dot_pair(s['q_mz'], s['q_int'], s['q_pmz'], s['l_mz'], s['l_int'], s['l_chg'], s['l_pmz'],
                                    z, tol, shift, 'ppm')
        one = _one(s['q_mz'], s['q_int'], s['q_pmz'], s['l_mz'], s['l_chg'], s['l_pmz'], z, tol, flags)
        assert not set(m[:, 0].tolist()) & set(one['src'].tolist()), t
        n_pairs += len(m)
        n_kept += one['count']
    assert n_pairs > 200 and n_kept > 200


# ------------------------------------------------------------------ configuration
def test_flag_defaults_the_sharding_error_and_the_hashes():
    cfg = Config()
    assert cfg.chimeric_search is False and cfg.chimeric_window == 2.0
    p = argparse.ArgumentParser()
    add_arguments(p)
    ns = p.parse_args([])
    assert ns.chimeric_search is False and ns.chimeric_window == 2.0
    ns = p.parse_args(['--chimeric_search', '--chimeric_window', '3.5'])
    cfg = Config.from_reference(ns)
    assert cfg.chimeric_search is True and cfg.chimeric_window == 3.5
    with pytest.raises(ValueError, match='chimeric_search.*sharded'):
        Config(chimeric_search=True, num_gpus=2)
    Config(chimeric_search=False, num_gpus=2)
    with pytest.raises(ValueError):
        Config(chimeric_window=-1.0)
    from ann_solo_amd.spectral_library import SpectralLibrary
    from ann_solo_amd import library_store
    out = []
    for kw in (dict(), dict(chimeric_search=True, chimeric_window=7.0)):          # no hash knows the switch
        sl = SpectralLibrary.__new__(SpectralLibrary)
        sl.config = Config.open_search(**kw)
        out.append((sl._get_hyperparameter_hash(), sl._get_index_hash(),
                    library_store.store_hash(sl.config, sl._get_hyperparameter_hash(), 'x')))
    assert out[0] == out[1]


def test_the_entry_point_is_declared_and_registered():
    import os
    from ann_solo_amd import _lib
    assert 'asl_deplete_batch' in _lib.EXPORTS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'annsolo_mi.h')).read()
    assert 'int asl_deplete_batch(const asl_peaks_t *queries, const asl_peaks_t *library,' in header
    assert os.path.exists(os.path.join(root, 'ann_solo_amd', 'csrc', 'deplete.hip'))


# ------------------------------------------------------------------ the engine on the oracle backend
def _engine(lib, kw, **more):
    from oracle import oracle_py as O
    from oracle_backend import OracleSpectralLibrary
    from ann_solo_amd.spectral_library import BatchResult

    class OracleChimericLibrary(OracleSpectralLibrary):
        """The oracle backend with the two keywords the residue level uses: per-query precursor intervals and
        the peak shifts of the call."""

        def _search_batch_local(self, queries, charge, mode, want_knn=False, device_out=False, pm_stride=None,
                                windows=None, shifts=None):
            if windows is None and shifts is None:
                return super()._search_batch_local(queries, charge, mode, want_knn, device_out, pm_stride)
            be = self._full[charge]
            Q = O.Spectra(*queries.numpy())
            l = be.pmz32.astype(np.float64)
            w = np.asarray(windows, np.float64)
            cands = [np.nonzero((w[i, 0] <= l) & (l <= w[i, 1]))[0].astype(np.int64) for i in range(Q.n)]
            saved = be.allow_shift
            be.allow_shift = saved if shifts is None else shifts
            try:
                r = be._best(Q, cands, pm_stride)
            finally:
                be.allow_shift = saved
            return BatchResult(r['best_row'], r['best_score'], r['n_candidates'], r['pm_count'], r['pm_pairs'])

    lib_np = lib.numpy()
    parts = {2: dict(lib_np=lib_np, pmz32=lib_np[4].astype(np.float32))}
    return OracleChimericLibrary(parts, Config.open_search(**kw, **more), 64, 4)


COLUMNS = ('charge', 'qrow', 'lib_row', 'score', 'q', 'open_level', 'chimeric_rank', 'explained_intensity',
           'delta_score', 'n_scored', 'expect', 'mod_mass', 'mod_site_lo')


@pytest.fixture
def on_the_oracle(O, monkeypatch):
    from ann_solo_amd import chimeric, spectrum_similarity
    from oracle_backend import oracle_cosines
    monkeypatch.setattr(spectrum_similarity, 'ssm_cosine', oracle_cosines)
    calls = []

    def deplete(*a, **k):
        calls.append(a[0].n)
        return R.torch_deplete_batch(*a, **k)
    monkeypatch.setattr(chimeric, 'deplete_batch', deplete)
    return calls


@pytest.mark.parametrize('isolation', (False, True))
def test_engine_finds_the_planted_partners(O, on_the_oracle, isolation, caplog):
    lib, qs, qmeta, lmeta, kw, plan = DC.world(isolation)
    off = _engine(lib, kw).search_packed(qs, qmeta, lmeta)
    assert not on_the_oracle                                    # switch off: no depletion
    assert not off.chimeric_rank.any() and np.isnan(off.explained_intensity).all()
    eng = _engine(lib, kw, chimeric_search=True)
    with caplog.at_level(logging.INFO):
        got = eng.search_packed(qs, qmeta, lmeta)
    assert on_the_oracle and 'spectra identified after the chimeric search' in caplog.text
    ref = DC.reference_level(O, off, lib, qs, qmeta, lmeta, eng.config)
    n0 = len(off)
    assert len(got) == n0 + len(ref)
    # the table is the cascade's own table ...
    for name in COLUMNS:
        a, b = getattr(got, name)[:n0], getattr(off, name)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    # ... followed by the reference's residue level
    assert got.qrow[n0:].tolist() == [r[0] for r in ref] and got.lib_row[n0:].tolist() == [r[1] for r in ref]
    assert got.score[n0:].tobytes() == np.array([r[2] for r in ref]).tobytes()
    assert got.explained_intensity[n0:].tobytes() == np.array([r[3] for r in ref]).tobytes()
    assert (got.chimeric_rank[n0:] == 1).all() and not got.open_level[n0:].any() and (got.q[n0:] == 0.0).all()
    # by construction: A at rank 0 and B at rank 1 for every planted query (what keeps the fixture meaningful)
    rank0 = {int(q): int(r) for q, r in zip(off.qrow, off.lib_row)}
    rank1 = {int(q): int(r) for q, r in zip(got.qrow[n0:], got.lib_row[n0:])}
    for i in range(DC.N_PLANTED):
        assert rank0[i] == plan[i][0] and rank1[i] == plan[i][1], i
    assert off.open_level[[list(off.qrow).index(i) for i in (1, 3)]].all()       # the odd ones: the open level
    # a residue whose best match is A's peptide again is dropped; a plain query leaves no valid residue
    for i in range(DC.N_PLANTED, DC.N_QUERIES - 1):
        assert rank0[i] == plan[i][0] and i not in rank1, i
    # the partner 2.0 m/z away: inside the isolation window only
    assert rank0[DC.FAR] == plan[DC.FAR][0]
    assert (rank1.get(DC.FAR) == plan[DC.FAR][1]) == isolation
    # the planted residues are B itself: nearly everything of the query that A does not explain
    ex = got.explained_intensity[n0:][[list(got.qrow[n0:]).index(i) for i in range(DC.N_PLANTED)]]
    assert np.allclose(ex, 1.0 / 1.36, atol=1e-5)
    rec = got[n0]
    assert rec.chimeric_rank == 1 and rec.explained_intensity == got.explained_intensity[n0]
    assert rec.query_identifier == got[list(off.qrow).index(int(got.qrow[n0]))].query_identifier
    assert got[0].chimeric_rank == 0 and np.isnan(got[0].explained_intensity)


def test_engine_level_options(O, on_the_oracle):
    """The level under the options of the standard level: a columnar scorer sees the residue SSMs with mode
    'std' after the drop; without an open level the residue level still runs."""
    lib, qs, qmeta, lmeta, kw, plan = DC.world()
    seen = []

    def scorer(table, mode):
        seen.append((mode, len(table), table.lib_row.copy()))
        table.q[:] = 0.0
    scorer.columnar = True
    got = _engine(lib, kw, chimeric_search=True).search_packed(qs, qmeta, lmeta, score_ssms=scorer)
    assert [m for m, _, _ in seen] == ['std', 'open', 'std']
    n_res = int((got.chimeric_rank == 1).sum())
    assert seen[2][1] == n_res >= DC.N_PLANTED
    same = {plan[i][1] for i in range(DC.N_PLANTED, DC.N_PLANTED + DC.N_SAME)}
    assert not same & set(seen[2][2].tolist())                 # dropped before the scorer saw them
    kw1 = dict(kw, precursor_tolerance_mass_open=None, precursor_tolerance_mode_open=None)
    one = _engine(lib, kw1, chimeric_search=True).search_packed(qs, qmeta, lmeta)
    r1 = {int(q): int(r) for q, r in zip(one.qrow[one.chimeric_rank == 1], one.lib_row[one.chimeric_rank == 1])}
    assert all(r1[i] == plan[i][1] for i in range(0, DC.N_PLANTED, 2)) and not any(i % 2 for i in r1)


def test_sharded_engine_refuses():
    from types import SimpleNamespace
    from ann_solo_amd.spectral_library import SpectralLibrary, SSMTable
    sl = SpectralLibrary.__new__(SpectralLibrary)
    sl.config = Config.open_search(chimeric_search=True)
    sl._dist = SimpleNamespace(world=2)
    with pytest.raises(ValueError, match='chimeric_search.*sharded'):
        sl._chimeric_level(SSMTable({}, {}), {}, {}, {}, None, None)

