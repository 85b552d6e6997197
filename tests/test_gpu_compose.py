"""The opt-in switches together, through the engine, on the planted world of tests/compose_cases.py.

Bases are configurations that change results (a pairwise covering array over index and mode, fragment tolerance
unit, open window and scorer); overlays are switches documented not to change them. Per (base, overlay set) one
engine and one search; then
  * the primary rows (chimeric_rank 0) of every overlay run are the rows of the base's run without overlays, to
    the byte, and every column no overlay of the set owns is what it is without overlays;
  * what an overlay owns is, in a run with others, what it is alone;
  * a kernel whose switch is off is not launched;
  * the run with everything on repeats itself on the same engine and leaves nothing behind for a fresh engine;
  * on the first base the table with everything on is held against the restatements the single-feature tests
    use: the oracle's search on the engine's own lists and its ranked matches (plain and distinct), the numpy
    score histogram, tests/localize_ref.py and the reference residue level of tests/deplete_cases.py."""
import copy
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import compose_cases as CC
from fake_reader import FakeReader

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# profile scope of the kernel an overlay switches on (csrc: ProfScope). The score histogram is counted inside the
# rescoring's own launches and has no scope: its switch-off check is the n_scored / expect columns
SCOPES = {'deplete': 'chimeric_search', 'localize': 'localize_modifications', 'tdc_qvalues': 'device_qvalues',
          'ssm_groups': 'device_groups'}
BASES = CC.bases()
# two-overlay runs the chimeric rows' alt_* / expect columns are held against
PAIRS = (('chimeric_search', 'distinct_matches'), ('chimeric_search', 'num_matches'), ('chimeric_search', 'score_stats'))


def _sets(base):     # (all but one: on the first two bases)
    return CC.overlay_sets(base, full=True, but_one=base in BASES[:2]) + list(PAIRS)


CASES = [(b, s) for b in BASES for s in _sets(b) if s]


def _every(base, distinct=True):
    """Every applicable overlay; ``distinct`` False: with the plain num_matches in place of distinct_matches."""
    every = CC.overlay_sets(base)[1]
    return every if distinct else tuple(sorted(set(every) - {'distinct_matches'} | {'num_matches'}))


def _id(v):
    return '-'.join(v) if v else 'none'


def _launches(name):
    from ann_solo_amd import _lib
    ms, n = C.c_double(), C.c_int64()
    _lib.lib().asl_profile_get(name.encode(), C.byref(ms), C.byref(n))
    return n.value


class Run:
    def __init__(self, table, again, launches, cfg, directory, qs, qmeta, lmeta, partitions):
        self.table, self.again, self.launches, self.cfg, self.directory = table, again, launches, cfg, directory
        self.qs, self.qmeta, self.lmeta, self.partitions = qs, qmeta, lmeta, partitions


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """run(base, names[, directory]) -> Run: the engine of that configuration, built in a directory of its own (or
    ``directory``: another run's, with its cached store and indexes) and searched once -- twice with every overlay
    on. Cached; the engines are shut down when their search is done, the last one at the end."""
    from ann_solo_amd import _lib
    from ann_solo_amd.config import Config
    from ann_solo_amd.library_store import pack_queries
    from ann_solo_amd.spectral_library import SpectralLibrary
    w = CC.world()
    L = _lib.lib()
    files = tmp_path_factory.mktemp('files')
    (files / 'queries.mgf').write_bytes(w['mgf'])
    cache, packed, engines = {}, {}, []

    def never(*a):
        raise AssertionError('the switch is on: the injected reader must not be called')

    def run(base, names, directory=None):
        key = (base, names, directory)
        if key in cache:
            return cache[key]
        cfg = Config.open_search(**dict(CC.base_kwargs(base), **CC.overlay_kwargs(names)))
        d = directory or str(tmp_path_factory.mktemp('lib'))
        if 'device_library' in names:
            path = os.path.join(d, 'lib.sptxt')
            with open(path, 'wb') as f:
                f.write(w['sptxt'])
            sl = SpectralLibrary(path, config=cfg, device=DEV, reader_factory=never, query_reader=never)
        else:
            sl = SpectralLibrary(FakeReader(w['library'], os.path.join(d, 'lib.splib')), config=cfg, device=DEV,
                                 query_reader=never)
        engines.append(sl)
        if not packed:          # the host route of the queries, once: the same for every configuration
            qs, qmeta = pack_queries(iter(w['queries']), sl.config, sl.device)
            packed.update(qs=qs, plain=qmeta, isolation=CC.add_isolation_windows(copy.deepcopy(qmeta)))
        qs, qmeta = packed['qs'], packed['isolation' if base[2] == 'isolation' else 'plain']
        tables = []
        L.asl_profile_reset()
        L.asl_profile_enable(1)
        try:
            for _ in range(2 if set(names) >= set(CC.overlay_sets(base)[1]) else 1):
                if 'device_mgf' in names:
                    tables.append(sl.search(str(files / 'queries.mgf')))
                else:
                    tables.append(sl.search_packed(qs, qmeta, sl.library_meta))
            sl.synchronize()
        finally:
            L.asl_profile_enable(0)
        launches = {scope: _launches(scope) for scope in SCOPES}
        for t in tables:        # the peak matches to the host while the engine lives
            for i in range(len(t)):
                t._peak_matches(i)
        out = Run(tables[0], tables[-1] if len(tables) > 1 else None, launches, cfg, d, qs, qmeta, sl.library_meta,
                  {z: (p.spectra.to('cpu'), np.asarray(p.precursor_mz)) for z, p in sl.partitions.items()})
        out.engine = sl if (base == CC.FIRST and names in (_every(base), _every(base, False))) else None
        if out.engine is None:
            sl.shutdown()
            engines.pop()
        cache[key] = out
        return out
    yield run
    for sl in engines:
        sl.shutdown()


def _primary(t):
    return np.nonzero(t.chimeric_rank == 0)[0]


def _alt_peaks_equal(a, ra, b, rb, what):
    assert a.n_alt == b.n_alt, what
    for i, j in zip(ra, rb):
        for r in range(1, a.n_alt + 1):
            assert np.array_equal(a.alt_peak_matches(int(i), r), b.alt_peak_matches(int(j), r)), (what, int(i), r)


def _counts(t, fdr):
    p = t.chimeric_rank == 0
    return dict(std=int((p & ~t.open_level).sum()), open=int(t.open_level.sum()),
                localised=int((t.mod_site_lo >= 0).sum()), chimeric=int((~p).sum()),
                expect=int(np.isfinite(t.expect).sum()),
                runner_up=int((t.alt_lib_row[:, 0] >= 0).sum()) if t.n_alt else 0, accepted=int((t.q < fdr).sum()))


# ------------------------------------------------------------------------------------------------ every case
@pytest.mark.parametrize('base,names', CASES, ids=[_id(b) + '+' + _id(s) for b, s in CASES])
def test_overlay_set(runs, base, names):
    none, got = runs(base, ()), runs(base, names)
    ref, t = none.table, got.table
    what = (_id(base), _id(names))
    assert len(ref) > 300 and not ref.chimeric_rank.any()
    # a kernel whose switch is off is not launched; one whose switch is on is
    for scope, overlay in SCOPES.items():
        assert (got.launches[scope] > 0) == (overlay in names), (what, scope, got.launches)
        assert none.launches[scope] == 0, (what, scope)
    # the primary rows: the same bytes as without overlays, peak matches included
    rows = _primary(t)
    assert len(rows) == len(ref) and np.array_equal(rows, np.arange(len(ref))), what
    CC.assert_rows_equal(t, ref, CC.PRIMARY, rows_a=rows, what=what)
    if ref.features.shape[1]:
        assert CC.column_bytes(t, 'features', rows) == CC.column_bytes(ref, 'features'), what
    # columns that no overlay of the set owns are the defaults of the run without overlays
    own = CC.owned(names)
    for col in CC.MOD_COLUMNS + CC.ALT_COLUMNS + CC.STAT_COLUMNS:
        if col not in own:
            assert CC.column_bytes(t, col, rows) == CC.column_bytes(ref, col), (what, col)
    if 'chimeric_search' not in names:
        assert len(t) == len(ref) and np.isnan(t.explained_intensity).all(), what
    else:
        extra = np.arange(len(ref), len(t))
        assert len(extra) >= 10 and (t.chimeric_rank[extra] == 1).all() and not t.open_level[extra].any(), what
        assert np.isfinite(t.explained_intensity[extra]).all() and np.isnan(t.explained_intensity[rows]).all(), what
        assert (t.mod_site_lo[extra] == -1).all() and (t.mod_site_hi[extra] == -1).all(), what
        for col in ('mod_mass', 'mod_site_score', 'mod_site_margin', 'mod_site_gain'):      # never localised
            assert np.isnan(getattr(t, col)[extra]).all(), (what, col)
        if not set(CC.ALT_COLUMNS) & own:       # the defaults of the columns nobody in the set owns
            assert t.alt_lib_row[extra].size == 0 and t.alt_score[extra].size == 0, what
            assert np.isnan(t.delta_score[extra]).all(), what
        if not set(CC.STAT_COLUMNS) & own:
            assert not t.n_scored[extra].any() and np.isnan(t.expect[extra]).all(), what
        # a second PSM names a query that has a first one, and another peptide
        first = {(int(z), int(r)): int(l) for z, r, l in zip(t.charge[rows], t.qrow[rows], t.lib_row[rows])}
        for i in extra:
            z = int(t.charge[i])
            assert got.lmeta[z][first[(z, int(t.qrow[i]))]]['peptide'] != got.lmeta[z][int(t.lib_row[i])]['peptide'], what
    # what an overlay owns is what it owns alone
    if len(names) > 1:
        for n in names:
            alone = runs(base, (n,)).table
            cols = CC.OVERLAYS[n]['owns']
            if cols:
                ra = _primary(alone)
                for col in cols:
                    assert CC.column_bytes(t, col, rows) == CC.column_bytes(alone, col, ra), (what, n, col)
                if cols == CC.ALT_COLUMNS:
                    _alt_peaks_equal(t, rows, alone, ra, (what, n))
            if n == 'chimeric_search':
                ea = np.arange(len(ref), len(alone))
                CC.assert_rows_equal(t, alone, CC.CHIMERIC_COLUMNS + ('charge',), rows_a=extra, rows_b=ea,
                                     what=(what, 'chimeric rows'))
                for m, cols in (('distinct_matches', CC.ALT_COLUMNS), ('num_matches', CC.ALT_COLUMNS),
                                ('score_stats', CC.STAT_COLUMNS)):
                    if m in names and tuple(sorted((n, m))) in PAIRS:
                        pair = runs(base, tuple(sorted((n, m)))).table
                        for col in cols:
                            assert CC.column_bytes(t, col, extra) == CC.column_bytes(pair, col, ea), (what, m, col)
                        if cols == CC.ALT_COLUMNS:
                            _alt_peaks_equal(t, extra, pair, ea, (what, m, 'chimeric rows'))
    # everything on: the run repeats itself on the same engine, every row materialises and answers every mzTab field
    if got.again is not None:
        import mztab_check as M
        again = got.again
        assert len(again) == len(t), what
        every = CC.PRIMARY + CC.MOD_COLUMNS + CC.ALT_COLUMNS + CC.STAT_COLUMNS + ('chimeric_rank', 'explained_intensity')
        CC.assert_rows_equal(again, t, every, what=(what, 'repeat'))
        _alt_peaks_equal(again, np.arange(len(t)), t, np.arange(len(t)), (what, 'repeat'))
        recs = t.materialize()
        assert len(recs) == len(t), what
        by_id = {}
        for i, s in enumerate(recs):
            one = t[i]
            for f in dataclasses.fields(s):
                a, b = getattr(one, f.name), getattr(s, f.name)
                if f.name == 'peak_matches':
                    assert np.array_equal(a, b) and np.array_equal(a, t._peak_matches(i)), (what, i)
                elif f.name == 'alternatives':
                    assert len(a) == len(b) == int((t.alt_lib_row[i] >= 0).sum()), (what, i)
                    for r, (x, y) in enumerate(zip(a, b)):
                        assert x[:2] == y[:2] and x[1] == t.alt_score[i, r] and np.array_equal(x[2], y[2]), (what, i, r)
                        assert np.array_equal(x[2], t.alt_peak_matches(i, r + 1)), (what, i, r)
                else:
                    assert a == b or (a != a and b != b), (what, i, f.name)
            # every mzTab field is what the table's own columns and the two metadata records say
            z = int(t.charge[i])
            qm, lm = t.query_meta[z][int(t.qrow[i])], t.library_meta[z][int(t.lib_row[i])]
            want = {'sequence': lm['peptide'], 'PSM_ID': qm['identifier'], 'search_engine_score[1]': float(t.score[i]),
                    'search_engine_score[2]': float(t.q[i]), 'retention_time': qm.get('retention_time'), 'charge': z,
                    'exp_mass_to_charge': qm['precursor_mz'], 'calc_mass_to_charge': lm['precursor_mz'],
                    'spectra_ref': 'ms_run[1]:index={}'.format(qm['index']),
                    'opt_ms_run[1]_cv_MS:1003062_spectrum_index': lm['identifier'],
                    'opt_ms_run[1]_cv_MS:1002217_decoy_peptide': '{:d}'.format(bool(lm.get('is_decoy', False)))}
            fields = M.record_fields(s)
            assert fields == {k: str(v) for k, v in want.items()}, (what, i, fields)
            assert 'None' not in (fields['sequence'], fields['PSM_ID'], fields['charge'], fields['spectra_ref']), what
            assert (s.chimeric_rank, s.n_scored) == (int(t.chimeric_rank[i]), int(t.n_scored[i])), (what, i)
            by_id.setdefault(fields['PSM_ID'], []).append(s)
        second = [v for v in by_id.values() if len(v) == 2]
        assert len(second) == len(extra) and max(len(v) for v in by_id.values()) == 2, what
        for a, b in second:         # the second PSM of a chimeric spectrum: the same spectrum, another sequence
            fa, fb = M.record_fields(a), M.record_fields(b)
            assert (a.chimeric_rank, b.chimeric_rank) == (0, 1) and a.sequence != b.sequence, what
            for col in ('PSM_ID', 'spectra_ref', 'charge', 'exp_mass_to_charge', 'retention_time'):
                assert fa[col] == fb[col], (what, col)
            assert np.isfinite(b.explained_intensity) and np.isnan(b.mod_mass), what
            assert np.isfinite(b.q) or b.is_decoy, what          # (the engine's scorers leave NaN on decoys, fdr.py)
        # the peak matches of a primary row are its own: they give its cosine back (scorers that learn a score of
        # their own overwrite it). A device sum of at most 80 positive fp64 products in another order: 80 * 2^-53
        if base[3] in ('none', 'tdc'):
            want = CC.cosines_of(t, rows, {z: q.to('cpu').numpy() for z, q in got.qs.items()},
                                 {z: p[0].numpy() for z, p in got.partitions.items()})
            fin = np.isfinite(t.score[rows])            # (the cosine gate leaves NaN on decoys)
            assert fin.sum() > 300 and np.all(np.abs(t.score[rows][fin] - want[fin]) <= 80 * 2.0 ** -53 * want[fin]), what
        print('compose', _id(base), _counts(t, got.cfg.fdr))


@pytest.mark.parametrize('base', BASES, ids=[_id(b) for b in BASES])
def test_a_fresh_engine_afterwards_is_unchanged(runs, base):
    """A search without overlays through a fresh engine on the library the engine with everything on left behind
    (its directory: the cached store and indexes) is the search without overlays."""
    left = runs(base, CC.overlay_sets(base)[1])      # (that engine read lib.sptxt; the fresh one is given the objects)
    fresh = runs(base, (), left.directory)
    ref = runs(base, ()).table
    assert len(fresh.table) == len(ref)
    CC.assert_rows_equal(fresh.table, ref, CC.PRIMARY + CC.MOD_COLUMNS + CC.ALT_COLUMNS + CC.STAT_COLUMNS,
                         what=(_id(base), 'fresh'))
    assert all(v == 0 for v in fresh.launches.values())


# ------------------------------------------------------------------------------------------------ the world
def test_world_is_not_vacuous_on_the_device(runs):
    """What the oracle-backed engine of tests/test_compose_cases_cpu.py does not serve, on the single-overlay runs
    of the first base; and the quantities it does serve, once more."""
    base = CC.FIRST
    none = runs(base, ()).table
    assert int((~none.open_level).sum()) >= 100 and int(none.open_level.sum()) >= 100
    assert int((runs(base, ('localize_modifications',)).table.mod_site_lo >= 0).sum()) >= 30
    assert int((runs(base, ('chimeric_search',)).table.chimeric_rank == 1).sum()) >= 10
    assert int(np.isfinite(runs(base, ('score_stats',)).table.expect).sum()) >= 100
    plain, distinct = runs(base, ('num_matches',)).table, runs(base, ('distinct_matches',)).table
    assert int((plain.alt_lib_row[:, 0] >= 0).sum()) >= 100 and int((distinct.alt_lib_row[:, 0] >= 0).sum()) >= 100
    differs = int((plain.alt_lib_row[:, 0] != distinct.alt_lib_row[:, 0]).sum())
    print('runner-up differs between num_matches and distinct_matches on', differs, 'rows')
    assert differs >= 1
    # a query without a charge is identified, once
    w = CC.world()
    unknown = {w['queries'][j].identifier for j in np.nonzero(w['kind'] == 'unknown')[0]}
    hits = [i for i in none.identifiers() if i in unknown]
    assert hits and len(set(hits)) == len(hits)
    # accepted and rejected SSMs under each scorer; decoys do win sometimes
    for scorer in ('tdc', 'svm', 'rf'):
        b = next(b for b in BASES if b[3] == scorer)
        r = runs(b, ())
        acc = r.table.q < r.cfg.fdr
        print(_id(b), 'accepted', int(acc.sum()), 'rejected', int((~acc).sum()), 'decoys', int(r.table.is_decoy().sum()))
        assert acc.any() and (~acc).any() and r.table.is_decoy().any()


# ------------------------------------------------------------------------------------------------ the anchor
def _window_rows(O, q_pmz, pmz32, z, tol, mode):
    return np.array([r for r in range(len(pmz32)) if O.precursor_ok(q_pmz, pmz32[r], z, tol, mode)], np.int64)


@pytest.mark.parametrize('distinct', (True, False), ids=('distinct_matches', 'num_matches'))
def test_everything_on_against_the_restatements(O, runs, distinct):
    """The first base (IVF-Flat fp32, Da, symmetric window, no scorer) with every overlay on, held directly against
    the restatements of the single-feature tests -- not against another run of the engine. The ranked matches are
    the oracle's best match applied three times: the winner deleted (num_matches: tests/test_gpu_topn.py's
    ``_oracle_ranks``, which ``oracle_ranks_distinct`` is when every row is ungrouped) or the winner's peptide
    (distinct_matches: tests/distinct_ref.py), with test_gpu_topn's assertions per rank."""
    import deplete_cases as DEP
    import localize_cases as LC
    import localize_ref
    import score_hist_ref as SH
    from distinct_ref import oracle_ranks_distinct
    from ann_solo_amd import score_stats, spectrum_similarity
    from ann_solo_amd.decoy_generator import default_fragment_charge
    base = CC.FIRST
    got = runs(base, _every(base, distinct))
    t, cfg, sl = got.table, got.cfg, got.engine
    assert cfg.num_matches == 3 and cfg.distinct_matches == distinct and cfg.score_stats and cfg.chimeric_search
    rows = _primary(t)
    tol = cfg.fragment_mz_tolerance
    n_alt = n_exp = n_loc = 0
    deltas = t.mass_diffs()
    for z, (lib, pmz32) in got.partitions.items():
        L, Q = O.Spectra(*lib.numpy()), O.Spectra(*got.qs[z].to('cpu').numpy())
        peps, group = {}, np.empty(lib.n, np.int64)
        for r in range(lib.n):
            group[r] = peps.setdefault(got.lmeta[z][r]['peptide'], len(peps)) if distinct else -1
        mine = rows[t.charge[rows] == z]
        # the open level's candidates: the ANN ids of the query inside the precursor window
        opened = mine[t.open_level[mine]]
        knn = {}
        if len(opened):
            import torch
            sel = got.qs[z].select(torch.as_tensor(t.qrow[opened]))
            res = sl._search_batch(sel, z, 'open', want_knn=True)
            knn = {int(i): np.unique(res.knn[k][res.knn[k] >= 0]) for k, i in enumerate(opened)}
            # the open level as tests/test_gpu_configs.py holds it: the oracle's search on the engine's own lists
            from oracle_backend import oracle_ivf
            ref = O.search_batch(O.Spectra(*sel.to('cpu').numpy()), L, pmz32, z, oracle_ivf(O, sl.partitions[z].index),
                                 cfg.num_candidates, cfg.num_probe, cfg.precursor_tolerance_mass_open,
                                 cfg.precursor_tolerance_mode_open, tol, True, pm_stride=res.pm_pairs.shape[1],
                                 want_knn=True)
            assert np.array_equal(res.knn, ref['knn_I']) and np.array_equal(res.pm_count, ref['pm_count'])
            assert np.array_equal(t.lib_row[opened], ref['best_row']), z
            for k, i in enumerate(opened):
                assert np.array_equal(t._peak_matches(int(i)), ref['pm_pairs'][k, :ref['pm_count'][k]]), (z, k)
        o, mz, it, *_ = got.qs[z].to('cpu').numpy()
        for i in mine:
            qr = int(t.qrow[i])
            if t.open_level[i]:
                ids = knn[int(i)]
                cand = ids[[O.precursor_ok(Q.precursor_mz[qr], pmz32[r], z, cfg.precursor_tolerance_mass_open,
                                           cfg.precursor_tolerance_mode_open) for r in ids]].astype(np.int64)
            else:
                cand = _window_rows(O, Q.precursor_mz[qr], pmz32, z, cfg.precursor_tolerance_mass,
                                    cfg.precursor_tolerance_mode)
            # the two levels and the runners-up: the oracle's best match, the winner (its peptide) deleted, three times
            ranks = oracle_ranks_distinct(O, Q, qr, L, cand, group, 3, tol, True)
            assert t.lib_row[i] == ranks[0][1] and np.array_equal(t._peak_matches(int(i)), ranks[0][3]), (z, qr)
            for r in range(1, 3):
                if r < len(ranks):
                    assert t.alt_lib_row[i, r - 1] == ranks[r][1] and t.alt_score[i, r - 1] == ranks[r][2], (z, qr, r)
                    assert np.array_equal(t.alt_peak_matches(int(i), r), ranks[r][3]), (z, qr, r)
                    n_alt += 1
                else:       # an empty rank
                    assert t.alt_lib_row[i, r - 1] == -1 and t.alt_score[i, r - 1] == 0.0, (z, qr, r)
                    assert len(t.alt_peak_matches(int(i), r)) == 0, (z, qr, r)
            assert t.delta_score[i] == ranks[0][2] - (ranks[1][2] if len(ranks) > 1 else 0.0), (z, qr)
            # n_scored / expect: the numpy histogram over the oracle's scores of the same candidates
            assert t.n_scored[i] == len(cand), (z, qr)
            hist = SH.hist_of(SH.pair_scores(O, Q, qr, L, cand, tol, True))
            best = np.array([ranks[0][2]])
            want = score_stats.expect_value(score_stats.loser_hist(hist[None, :], best), best)[0]
            assert (np.isnan(want) and np.isnan(t.expect[i])) or want == t.expect[i], (z, qr, want, t.expect[i])
            n_exp += int(np.isfinite(want))
            # the mod_* columns: tests/localize_ref.py on the processed query spectrum
            delta = deltas[i] if t.open_level[i] else 0.0
            cols = (t.mod_mass[i], t.mod_site_score[i], t.mod_site_margin[i], t.mod_site_gain[i])
            if not (t.open_level[i] and abs(delta) >= tol):
                assert np.isnan(cols).all() and t.mod_site_lo[i] == t.mod_site_hi[i] == -1, (z, qr)
                continue
            pep = LC.parse(got.lmeta[z][int(t.lib_row[i])]['peptide'])
            r = localize_ref.localize_ref(mz[o[qr]:o[qr + 1]], it[o[qr]:o[qr + 1]], pep.masses, pep.nterm, pep.cterm,
                                          default_fragment_charge(z), delta, tol, 'Da')
            assert (t.mod_site_lo[i], t.mod_site_hi[i]) == (r['best_lo'], r['best_hi']), (z, qr)
            want = (delta, r['best_score'], r['best_score'] - r['runner_score'], r['best_score'] - r['none_score'])
            assert LC.bits(list(cols)).tolist() == LC.bits(list(want)).tolist(), (z, qr, cols, want)
            n_loc += 1
    print('anchored: runners-up', n_alt, 'finite expect', n_exp, 'localised', n_loc)
    assert n_alt >= 100 and n_exp >= 100 and n_loc >= 30
    # the chimeric rows of charge 2 against the reference residue level on the engine's own primary rows
    lib2 = got.partitions[2][0]
    two = t.take(rows[t.charge[rows] == 2])
    ref = DEP.reference_level(O, two, lib2, {2: got.qs[2].to('cpu')}, got.qmeta, got.lmeta, cfg,
                              cosines=spectrum_similarity.ssm_cosine)
    extra = np.arange(len(rows), len(t))
    extra = extra[t.charge[extra] == 2]
    assert len(ref) >= 10 and len(extra) == len(ref)
    assert t.qrow[extra].tolist() == [r[0] for r in ref] and t.lib_row[extra].tolist() == [r[1] for r in ref]
    assert t.score[extra].tobytes() == np.array([r[2] for r in ref]).tobytes()
    assert t.explained_intensity[extra].tobytes() == np.array([r[3] for r in ref]).tobytes()
    # what rides along with a chimeric row is its own residue's: the candidates counted are the rows of ITS window
    # (the windows differ from query to query), the runners-up lie inside it and are other peptides (distinct_matches)
    # or other rows (num_matches)
    n_run = 0
    for i in np.arange(len(rows), len(t)):
        z, qr = int(t.charge[i]), int(t.qrow[i])
        pmz = float(got.qs[z].precursor_mz[qr])
        col = got.partitions[z][1].astype(np.float64)
        inside = (pmz - cfg.chimeric_window / 2.0 <= col) & (col <= pmz + cfg.chimeric_window / 2.0)
        assert t.n_scored[i] == int(inside.sum()), (z, qr)
        name = (lambda row: got.lmeta[z][row]['peptide']) if distinct else (lambda row: row)
        seen = [name(int(t.lib_row[i]))]
        last = np.inf
        for r in range(t.n_alt):
            row = int(t.alt_lib_row[i, r])
            if row < 0:
                assert (t.alt_lib_row[i, r:] == -1).all() and not t.alt_score[i, r:].any(), (z, qr)
                break
            assert inside[row] and name(row) not in seen and t.alt_score[i, r] <= last, (z, qr, r)
            seen.append(name(row))
            last = t.alt_score[i, r]
            assert (len(t.alt_peak_matches(int(i), r + 1)) > 0) == (t.alt_score[i, r] > 0.0), (z, qr, r)
            n_run += 1
    assert n_run >= 10
