"""The composition tests' own ground, without a GPU: the list of bases is a pairwise covering array that ``Config``
accepts with every applicable overlay set, the refusals are the documented ones, the comparison rules are
consistent, and the planted world (tests/compose_cases.py) is not vacuous -- measured on the oracle-backed engine
with the depletion, the score histogram and the localisation answered by their numpy restatements. What that
engine does not serve (runners-up, decoys and the scorers) is asserted by tests/test_gpu_compose.py on the
single-overlay runs of the first base."""
import itertools

import numpy as np
import pytest

import compose_cases as CC
from ann_solo_amd.config import Config


# ------------------------------------------------------------------------------------------------ the bases
def test_bases_cover_every_accepted_pair():
    bases = CC.bases()
    assert bases[0] == CC.FIRST and len(set(bases)) == len(bases)
    covered = set().union(*(CC.pairs_of(b) for b in bases))
    wanted = CC.all_pairs()
    assert wanted <= covered
    # no pair of two axes is refused today; the refusals lie inside the index axis (asserted below)
    n_all = sum(len(CC.AXES[a]) * len(CC.AXES[b]) for a, b in itertools.combinations(CC.AXIS_NAMES, 2))
    assert len(wanted) == n_all == 98
    # the two largest axes have 8 and 4 values: no covering array is shorter than their product
    assert len(bases) == 32


def test_config_accepts_every_base_with_every_overlay_set():
    n = 0
    for base in CC.bases():
        kw = CC.base_kwargs(base)
        for names in CC.overlay_sets(base, full=True, but_one=True):
            cfg = Config.open_search(**dict(kw, **CC.overlay_kwargs(names)))
            assert cfg.device_decoys and cfg.precursor_tolerance_mass_open == 300.0
            n += 1
        if base[3] == 'none':       # the two overlays of the FDR step are refused without it: the documented error
            assert 'device_qvalues' not in CC.applicable(base) and 'device_groups' not in CC.applicable(base)
            for name in ('device_qvalues', 'device_groups'):
                with pytest.raises(ValueError, match=name + '.*device_fdr'):
                    Config.open_search(**dict(kw, **CC.overlay_kwargs((name,))))
        else:
            assert {'device_qvalues', 'device_groups'} <= set(CC.applicable(base))
    assert n > 32 * 12


def test_pairs_that_config_refuses_stay_refused():
    for kw, words in ((dict(index='winflat', refine_k=32), ('winflat', 'refine_k')),
                      (dict(index='ivfpq', ann_window='pre', refine_k=32), ('pre', 'refine_k')),
                      (dict(index='ivfflat', ann_window='pre'), ('pre', 'ivfpq')),
                      (dict(index='ivfflat', pq_by_residual=False), ('pq_by_residual', 'ivfpq')),
                      (dict(device_fdr=True, model='rf'), ('rf',)),
                      (dict(model='rf', device_forest=True), ('device_forest', 'device_fdr'))):
        with pytest.raises(ValueError) as e:
            Config.open_search(**dict(CC.ENGINE, **kw))
        assert all(w in str(e.value) for w in words), (kw, str(e.value))


@pytest.mark.parametrize('name', CC.SHARDED_REFUSED)
def test_every_overlay_is_refused_on_a_sharded_index(name):
    """On the first base -- Da, symmetric window, no scorer: nothing of its own that a sharded index refuses -- the
    ValueError is the overlay's own and names its switch. ``distinct_matches`` is asked at num_matches = 1: beside
    num_matches = 3 that switch's refusal comes first (asserted too). ``device_qvalues`` / ``device_groups`` exist
    only with ``device_fdr``, which a sharded index refuses before them: that refusal is what a user meets, and it
    is asserted; their own cannot be reached through ``Config`` today, so what is held is that ``__post_init__``
    still states it, behind the check of ``device_fdr``."""
    base = CC.FIRST
    assert Config.open_search(**CC.base_kwargs(base), num_gpus=2).num_gpus == 2       # the base itself shards
    kw = dict(CC.base_kwargs(base), **CC.overlay_kwargs((name,)))
    if name == 'distinct_matches':
        with pytest.raises(ValueError, match='num_matches.*sharded'):
            Config.open_search(**kw, num_gpus=2)
        kw['num_matches'] = 1
    if name in ('device_qvalues', 'device_groups'):
        import inspect
        kw['device_fdr'] = True
        Config.open_search(**kw)
        with pytest.raises(ValueError, match='device_fdr.*sharded'):
            Config.open_search(**kw, num_gpus=2)
        src = inspect.getsource(Config.__post_init__)
        own = src.index(f"'{name} does not run on a sharded index (num_gpus > 1)'")
        assert src.index("'device_fdr does not run on a sharded index (num_gpus > 1)'") < own
        assert src.rindex(f'if self.{name}:', 0, own) < src.rindex('int(self.num_gpus) > 1', 0, own)
        return
    Config.open_search(**kw)
    with pytest.raises(ValueError, match=name + '.*sharded'):
        Config.open_search(**kw, num_gpus=2)


def test_rules_are_consistent():
    cols = set(CC.PRIMARY) | set(CC.MOD_COLUMNS) | set(CC.ALT_COLUMNS) | set(CC.STAT_COLUMNS) | set(CC.CHIMERIC_COLUMNS)
    from ann_solo_amd.spectral_library import SSMTable
    t = SSMTable({}, {}, 2)
    for c in cols:
        assert hasattr(t, c), c
    for name, o in CC.OVERLAYS.items():
        assert not set(o['owns']) & set(CC.PRIMARY), name           # nobody owns a primary column
        for k in o['config']:
            assert hasattr(Config(), k), k
    for a, b in itertools.combinations(CC.OVERLAYS, 2):             # two overlays own the same column only if exclusive
        if set(CC.OVERLAYS[a]['owns']) & set(CC.OVERLAYS[b]['owns']):
            assert CC.EXCLUSIVE.get(a) == b, (a, b)
    every = CC.overlay_sets(CC.bases()[1])[1]
    assert set(every) == set(CC.OVERLAYS) - set(CC.EXCLUSIVE)
    assert CC.overlay_kwargs(every)['distinct_matches'] and CC.overlay_kwargs(every)['num_matches'] == 3


# ------------------------------------------------------------------------------------------------ the world
def test_world_texts_and_objects_agree():
    w = CC.world()
    n = CC.N_PLAIN2 + CC.N_PLAIN3 + CC.N_MOD + CC.N_PAIRS + CC.N_FOREIGN + CC.N_UNKNOWN + 2
    assert len(w['queries']) == n == len(w['kind']) and len(w['library']) == CC.N_LIB2 + CC.N_LIB3
    assert sum(s.precursor_charge == 3 for s in w['library']) == CC.N_LIB3
    assert sum(s.precursor_charge is None for s in w['queries']) == CC.N_UNKNOWN
    assert all(s.peptide for s in w['library'])
    peps = [s.peptide for s in w['library']]
    assert len(set(peps)) == len(peps) - CC.N_REPEAT
    empty = w['queries'][int(np.nonzero(w['kind'] == 'empty')[0][0])]
    assert len(empty.mz) == 0
    # the wide query keeps more than 64 non-zero hash components
    from ann_solo_amd.spectrum import get_dim
    cfg = Config.open_search(**CC.ENGINE)
    lib_np, lmeta, qs, qmeta = CC.host_packs(w, cfg)
    wide = w['queries'][int(np.nonzero(w['kind'] == 'wide')[0][0])].identifier
    row = [m['identifier'] for m in qmeta[2]].index(wide)
    o, mz, *_ = qs[2].numpy()
    _, min_bound, _ = get_dim(cfg.min_mz, cfg.max_mz, cfg.bin_size)
    bins = np.unique(np.floor((mz[o[row]:o[row + 1]].astype(np.float64) - min_bound) / cfg.bin_size))
    assert len(bins) > 64
    assert empty.identifier not in [m['identifier'] for m in qmeta[2]]      # dropped by the preprocessing
    # unknown charges: one identifier in both charge sets
    both = set(m['identifier'] for m in qmeta[2]) & set(m['identifier'] for m in qmeta[3])
    assert len(both) == CC.N_UNKNOWN


def _engine(O, lib_np, cfg):
    from oracle_backend import OracleSpectralLibrary
    import score_hist_ref as SH
    from ann_solo_amd.spectral_library import BatchResult, TopnBatchResult

    class OracleComposeLibrary(OracleSpectralLibrary):
        """The oracle backend with per-query precursor intervals, the call's own peak shifts and the histogram
        call (n_best = 1), all answered by the oracle over the window's rows."""

        def _cands(self, be, Q, mode, windows):
            l = be.pmz32.astype(np.float64)
            if windows is not None:
                w = np.asarray(windows, np.float64)
                return [np.nonzero((w[i, 0] <= l) & (l <= w[i, 1]))[0].astype(np.int64) for i in range(Q.n)]
            tol_val, tol_mode = be.window_tol[mode]
            return [np.nonzero(be._window_ok(Q.precursor_mz[i], tol_val, tol_mode))[0].astype(np.int64)
                    for i in range(Q.n)]

        def _search_batch_local(self, queries, charge, mode, want_knn=False, device_out=False, pm_stride=None,
                                windows=None, shifts=None):
            if charge not in self.partitions:
                return None
            be = self._full[charge]
            Q = O.Spectra(*queries.numpy())
            saved = be.allow_shift
            be.allow_shift = saved if shifts is None else shifts
            try:
                r = be._best(Q, self._cands(be, Q, mode, windows), pm_stride)
            finally:
                be.allow_shift = saved
            return BatchResult(r['best_row'], r['best_score'], r['n_candidates'], r['pm_count'], r['pm_pairs'])

        def search_batch_topn(self, queries, charge, mode, n_best, want_knn=False, device_out=False, pm_stride=None,
                              distinct=False, windows=None, score_hist=False, shifts=None):
            assert n_best == 1 and score_hist
            res = self._search_batch_local(queries, charge, mode, windows=windows, shifts=shifts)
            if res is None:
                return None
            be = self._full[charge]
            Q = O.Spectra(*queries.numpy())
            shift = be.allow_shift if shifts is None else shifts
            hist = np.stack([SH.hist_of(SH.pair_scores(O, Q, i, be.L, rows, be.frag_tol, shift))
                             for i, rows in enumerate(self._cands(be, Q, mode, windows))])
            assert np.array_equal(hist.sum(axis=1), res.n_candidates)
            return TopnBatchResult(res.best_row[:, None], res.best_score[:, None], res.n_candidates,
                                   res.pm_count[:, None], res.pm_pairs[:, None], None, hist)

    parts = {z: dict(lib_np=p, pmz32=p[4].astype(np.float32)) for z, p in lib_np.items()}
    return OracleComposeLibrary(parts, cfg, 64, 8)


def _host_localize(spectra, seq_offsets, residue_mass, nterm, cterm, zmax, delta, tol, unit, device='cpu'):
    import localize_ref
    from ann_solo_amd import localize as lz
    o, mz, it, *_ = spectra.numpy()
    out = {k: [] for k in lz.SSM_KEYS}
    for i in range(spectra.n):
        r = localize_ref.localize_ref(mz[o[i]:o[i + 1]], it[o[i]:o[i + 1]], residue_mass[seq_offsets[i]:seq_offsets[i + 1]],
                                      nterm[i], cterm[i], zmax[i], delta[i], tol, unit)
        for k in lz.SSM_KEYS:
            out[k].append(r[k])
    return {k: np.asarray(v) for k, v in out.items()}


@pytest.fixture(scope='module')
def reference_tables(O):
    """The world through the oracle-backed engine ('bf', Da, symmetric window, no scorer): switches off, and
    score_stats + localize_modifications + chimeric_search on."""
    import deplete_ref
    from ann_solo_amd import chimeric, localize, spectrum_similarity
    from oracle_backend import oracle_cosines
    mp = pytest.MonkeyPatch()
    mp.setattr(spectrum_similarity, 'ssm_cosine', oracle_cosines)
    mp.setattr(chimeric, 'deplete_batch', deplete_ref.torch_deplete_batch)
    mp.setattr(localize, 'localize_batch', _host_localize)
    try:
        w = CC.world()
        kw = dict(CC.ENGINE, mode='bf')
        off_cfg = Config.open_search(**kw)
        lib_np, lmeta, qs, qmeta = CC.host_packs(w, off_cfg)
        off = _engine(O, lib_np, off_cfg).search_packed(qs, qmeta, lmeta)
        on_cfg = Config.open_search(**kw, score_stats=True, localize_modifications=True, chimeric_search=True)
        on = _engine(O, lib_np, on_cfg).search_packed(qs, qmeta, lmeta)
        yield w, off, on, qmeta, lmeta, lib_np, {z: q.numpy() for z, q in qs.items()}
    finally:
        mp.undo()


def test_world_is_not_vacuous_on_the_reference(reference_tables):
    w, off, on, qmeta, lmeta, lib_np, q_np = reference_tables
    primary = on.chimeric_rank == 0
    n_std, n_open = int((~on.open_level & primary).sum()), int(on.open_level.sum())
    n_loc, n_chim = int((on.mod_site_lo >= 0).sum()), int((on.chimeric_rank == 1).sum())
    n_expect = int(np.isfinite(on.expect).sum())
    print('reference: standard', n_std, 'open', n_open, 'localised', n_loc, 'chimeric', n_chim, 'finite expect', n_expect)
    assert n_std >= 100 and n_open >= 100 and n_loc >= 30 and n_chim >= 10 and n_expect >= 100
    # the planted things are what is found: the modified queries name their own library spectrum and site
    ident = {(int(z), int(r)): i for i, (z, r) in enumerate(zip(on.charge, on.qrow)) if primary[i]}
    by_id = {m['identifier']: (z, r) for z, metas in qmeta.items() for r, m in enumerate(metas)}
    right = sited = 0
    for j in np.nonzero(w['kind'] == 'mod')[0]:
        i = ident.get(by_id[w['queries'][j].identifier])
        rec, site, delta = w['planted'][j]
        if i is not None and on.open_level[i] and lmeta[2][int(on.lib_row[i])]['identifier'] == str(rec):
            right += 1
            sited += int(on.mod_site_lo[i] <= site <= on.mod_site_hi[i] and abs(on.mod_mass[i] - delta) < 0.01)
    assert right >= 100 and sited >= 30, (right, sited)
    # the mixtures: both twins, one at each rank
    chim = {int(r): int(l) for r, l in zip(on.qrow[on.chimeric_rank == 1], on.lib_row[on.chimeric_rank == 1])}
    both = 0
    for j in np.nonzero(w['kind'] == 'mix')[0]:
        z, r = by_id[w['queries'][j].identifier]
        i = ident.get((z, r))
        if i is not None and r in chim:
            got = {lmeta[2][int(on.lib_row[i])]['identifier'], lmeta[2][chim[r]]['identifier']}
            both += got == {str(v) for v in w['planted'][j]}
    assert both >= 10, both
    # at least one query without a charge is identified, at the charge of its library spectrum
    unknown = {w['queries'][j].identifier: w['planted'][j][0] for j in np.nonzero(w['kind'] == 'unknown')[0]}
    hits = [i for i in range(len(on)) if primary[i] and qmeta[int(on.charge[i])][int(on.qrow[i])]['identifier'] in unknown]
    assert hits and len({qmeta[int(on.charge[i])][int(on.qrow[i])]['identifier'] for i in hits}) == len(hits)
    good = [i for i in hits if lmeta[int(on.charge[i])][int(on.lib_row[i])]['identifier'] ==
            str(unknown[qmeta[int(on.charge[i])][int(on.qrow[i])]['identifier']])]
    assert len(good) >= 1 and {int(on.charge[i]) for i in good} == {2, 3}


def test_composition_on_the_reference_engine(reference_tables):
    """The three overlays the oracle-backed engine serves, together: the primary rows are the rows without them,
    to the byte (the host-side composition: top-n entry with windows and shifts, the rank-0 filter, concat, the
    localisation behind the appended rows)."""
    w, off, on, qmeta, lmeta, lib_np, q_np = reference_tables
    n0 = len(off)
    assert (on.chimeric_rank[:n0] == 0).all() and (on.chimeric_rank[n0:] == 1).all() and len(on) > n0
    CC.assert_rows_equal(on, off, CC.PRIMARY, rows_a=np.arange(n0), what='score_stats + localize + chimeric')
    assert not on.open_level[n0:].any() and (on.mod_site_lo[n0:] == -1).all() and np.isnan(on.mod_mass[n0:]).all()
    assert (on.n_scored > 0).all() and np.isfinite(on.explained_intensity[n0:]).all()
    assert np.isnan(on.explained_intensity[:n0]).all()
    recs = on.materialize()
    assert len(recs) == len(on) and recs[n0].chimeric_rank == 1
    # not only equal to the run without: every primary row's peak matches are its own (they give its score back) ...
    rows = np.arange(n0)
    assert on.score[rows].tobytes() == CC.cosines_of(on, rows, q_np, lib_np).tobytes()
    # ... and a second PSM names a query that has a first one, with another peptide
    first = {(int(z), int(r)): int(l) for z, r, l in zip(on.charge[rows], on.qrow[rows], on.lib_row[rows])}
    for i in range(n0, len(on)):
        z = int(on.charge[i])
        assert lmeta[z][first[(z, int(on.qrow[i]))]]['peptide'] != lmeta[z][int(on.lib_row[i])]['peptide']
