"""Subset search (asl_index_set_selector / asl_index_search_selected, asl_library_set_selection,
``SpectralLibrary.set_search_subset``): the scans choose their k among the SELECTED vectors of the probed
lists. Every comparison is against the oracle over an index that holds, in the same lists, only the
selected vectors (tests/selector_ref.py) -- ids equal, score bits equal -- and through the fused calls
against the oracle's whole batch over that index and a key column with NaN for the unselected rows:
best_row, best_score, n_candidates, pm_count, pm_pairs and knn equal."""
import numpy as np
import pytest

import raw_pq_ref as RAW
import selector_ref as R
from test_gpu_window_scan import _queries, _spectra_rows, _tie_library, _window_mask

pytestmark = pytest.mark.gpu

FIELDS = ('best_row', 'best_score', 'n_candidates', 'pm_count', 'pm_pairs')
KINDS = ('pq', 'pq_raw', 'flat', 'fx22')
NLIST, NPROBE = 16, 8
ERR_STATE = 'error -3'


def _encode(O, spectra):
    o, mz, it, *_ = spectra.numpy()
    _, min_bound, _ = O.get_dim(11, 2010, 0.04)
    return O.encode_batch(mz, it, o, min_bound, 0.04, 800)


def _new_index(kind, xb, nlist=NLIST, niter=4, m=32):
    from ann_solo_amd import faiss_compat as faiss
    if kind in ('pq', 'pq_raw'):
        idx = faiss.IndexIVFPQ(faiss.IndexFlatIP(xb.shape[1]), xb.shape[1], nlist, m, 8)
        if kind == 'pq_raw':
            idx.by_residual = False
    else:
        idx = faiss.IndexIVFFlat(faiss.IndexFlatIP(xb.shape[1]), xb.shape[1], nlist,
                                 storage='fx22' if kind == 'fx22' else 'fp32')
    idx.set_niter(niter)
    idx.train(xb)
    idx.add(xb)
    idx.nprobe = NPROBE
    return idx


def _reference(O, kind, ivf, xq, k, nprobe, keep):
    if kind == 'pq_raw':      # by_residual off: the oracle's codes scored with a zero coarse term
        return RAW.raw_search(O, xq, ivf.centroids, ivf, k, nprobe, keep=np.broadcast_to(keep, (len(xq), len(keep))))
    return R.search_selected(O, ivf, xq, k, nprobe, keep)


@pytest.fixture(scope='module')
def tie(O):
    lib0, aux, lib = _tie_library()
    q = _queries(lib0, aux, 48, seed=72, with_copies=8)
    return dict(lib0=lib0, aux=aux, lib=lib, q=q, xb=_encode(O, lib), xq=_encode(O, q), idx={}, ivf={})


def _get(O, tie, kind):
    if kind not in tie['idx']:
        tie['idx'][kind] = _new_index(kind, tie['xb'])
        tie['ivf'][kind] = R.host_ivf(O, tie['idx'][kind])
    return tie['idx'][kind], tie['ivf'][kind]


def _index_masks(idx, ivf, xq):
    """name -> keep by id. The position masks come from the lists the index holds."""
    n = len(ivf.ids)
    ids = np.arange(n)
    off = ivf.list_offsets
    pos = np.concatenate([np.arange(off[l + 1] - off[l]) for l in range(ivf.nlist)])       # position inside its list
    length = np.repeat(np.diff(off), np.diff(off))
    lst = np.repeat(np.arange(ivf.nlist), np.diff(off))
    by_pos = lambda sel: np.isin(ids, ivf.ids[sel])
    _, cI = idx.coarse(xq[:1], NPROBE)
    ties = np.ones(n, bool)
    ties[:400] = ids[:400] % 2 == 0                 # the 400 copies of row 0, every other one
    return {
        'every3': ids % 3 == 0, 'every16': ids % 16 == 0, 'rand30': np.random.default_rng(1).random(n) < 0.3,
        'all': np.ones(n, bool), 'none': np.zeros(n, bool),
        'tile_edges': by_pos((pos % 64 == 0) | (pos % 64 == 63)),
        'list_out': by_pos(lst != int(cI[0, 0])),   # the first query's best list is wholly unselected
        'last_tile': by_pos(pos >= 64 * ((length - 1) // 64)),
        'ties_half': ties,
    }


@pytest.mark.parametrize('kind', KINDS)
def test_index_level_matches_the_filtered_oracle(O, tie, kind):
    idx, ivf = _get(O, tie, kind)
    xq = tie['xq']
    masks = _index_masks(idx, ivf, xq)
    plain = {k: idx.search(xq, k) for k in (64, 256, 1024)}
    grew = short = 0
    for name, keep in masks.items():
        idx.set_selector(keep)
        for k in (64, 256, 1024):
            got = idx.search_selected(xq, k)
            R.assert_rows_equal(got, _reference(O, kind, ivf, xq, k, NPROBE, keep), (kind, name, k))
            hit = got[1][got[1] >= 0]
            assert keep[hit].all(), (kind, name, k)
            if name == 'all':
                R.assert_rows_equal(got, plain[k], (kind, name, k))
            if name == 'none':
                assert (got[1] == -1).all()
            if name == 'every3' and k == 256:       # a filter behind the top-k would leave these
                post = R.post_filtered(plain[k][1], keep)
                grew = sum(len(set(got[1][i][got[1][i] >= 0].tolist())) > len(post[i]) for i in range(len(xq)))
            if name == 'every16' and k == 256:
                short = int((got[1] < 0).any(1).sum())
        if name == 'ties_half':                     # ties at the k-th score: the selected copies of row 0
            _, I = idx.search_selected(xq[:8], 64)
            assert (I >= 0).all() and (I < 400).all() and (I % 2 == 0).all()
    assert grew > len(xq) // 2 and short > len(xq) // 2
    # a plain search ignores the selector
    idx.set_selector(masks['every16'])
    R.assert_rows_equal(idx.search(xq, 256), plain[256], kind)
    idx.set_selector(None)
    with pytest.raises(Exception, match=ERR_STATE):
        idx.search_selected(xq, 64)


def test_selector_and_window_together(O, tie):
    idx, ivf = _get(O, tie, 'pq')
    xq, q = tie['xq'], tie['q']
    q_pmz = q.numpy()[4].astype(np.float64)
    key0 = np.ascontiguousarray(tie['lib'].numpy()[4], np.float32)
    key_nan = key0.copy()
    key_nan[::7] = np.nan
    n = len(key0)
    masks = {'every3': np.arange(n) % 3 == 0, 'rand30': np.random.default_rng(1).random(n) < 0.3}
    some = 0
    for key, tol, mode in ((key0, 250.0, 'Da'), (key0, 10.0, 'ppm'), (key0, -1.0, 'Da'), (key_nan, 250.0, 'Da')):
        idx.set_window_key(key)
        for name, keep in masks.items():
            idx.set_selector(keep)
            D, I = idx.search_selected(xq, 256, window=(q_pmz, 2, tol, mode))
            for i in range(len(xq)):
                both = keep & _window_mask(q_pmz[i], key, 2, tol, mode)
                rD, rI = R.search_selected(O, ivf, xq[i:i + 1], 256, NPROBE, both)
                R.assert_rows_equal((D[i:i + 1], I[i:i + 1]), (rD, rI), (tol, mode, name, i))
            if tol < 0:
                assert (I == -1).all()
            else:
                some += int((I >= 0).sum())
    assert some > 0
    idx.set_selector(None)


@pytest.mark.parametrize('kind', ['pq', 'flat'])
def test_wide_probe_lists(O, kind):
    """nprobe above 512: the two-probes-per-thread instantiations."""
    from ann_solo_amd import synthetic
    lib, aux = synthetic.make_library(6000, seed=81, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, 16, seed=82, charge=2)
    xb, xq = _encode(O, lib), _encode(O, q)
    idx = _new_index(kind, xb, nlist=640, niter=2)
    idx.nprobe = 520
    ivf = R.host_ivf(O, idx)
    for keep in (np.arange(len(xb)) % 3 == 0, np.random.default_rng(2).random(len(xb)) < 0.1):
        idx.set_selector(keep)
        R.assert_rows_equal(idx.search_selected(xq, 64), R.search_selected(O, ivf, xq, 64, 520, keep), kind)


# ------------------------------------------------------------------ fused paths, through SpectralLibrary

def _config(index='ivfpq', window='post', tol=250.0, **kw):
    from ann_solo_amd.spectral_library import Config
    return Config.open_search(num_list=NLIST, num_probe=NPROBE, num_candidates=256, index=index, kmeans_niter=4,
                              precursor_tolerance_mass_open=tol, precursor_tolerance_mode_open='Da',
                              ann_window=window, **kw)


def _oracle_batch(O, sl, q, keep, tol, per_query_window=False):
    """The oracle's batch over the index filtered by `keep` and the key column with NaN where unselected
    (per_query_window: the 'pre' scan -- filtered by the selection AND each query's window)."""
    part = sl.partitions[2]
    L = O.Spectra(*part.spectra.to('cpu').numpy())
    ivf = R.host_ivf(O, part.index)
    key = R.key_with_selection(part.precursor_mz, keep)
    stride = 64
    if not per_query_window:
        return O.search_batch(O.Spectra(*q.numpy()), L, key, 2, R.filtered(O, ivf, keep), 256, NPROBE, tol, 'Da',
                              0.02, True, pm_stride=stride, want_knn=True)
    q_pmz = q.numpy()[4].astype(np.float64)
    rows = []
    for i in range(q.n):
        both = keep & _window_mask(q_pmz[i], part.precursor_mz, 2, tol, 'Da')
        rows.append(O.search_batch(_spectra_rows(O, q, [i]), L, key, 2, R.filtered(O, ivf, both), 256, NPROBE, tol,
                                   'Da', 0.02, True, pm_stride=stride, want_knn=True))
    return {f: np.concatenate([r[f] for r in rows]) for f in rows[0]}


def _assert_batch(res, ref, what=''):
    assert np.array_equal(res.knn, ref['knn_I']), what
    for f, g in (('n_candidates', 'n_cand'), ('best_row', 'best_row'), ('best_score', 'best_score'),
                 ('pm_count', 'pm_count')):
        assert np.array_equal(getattr(res, f), ref[g]), (what, f)
    for i in range(len(res.pm_count)):
        c = res.pm_count[i]
        assert np.array_equal(res.pm_pairs[i, :c], ref['pm_pairs'][i, :c]), (what, i)


def _same_fields(a, b, what=''):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        x = x.cpu().numpy() if hasattr(x, 'cpu') else x
        y = y.cpu().numpy() if hasattr(y, 'cpu') else y
        assert np.array_equal(x.astype(y.dtype), y), (what, f)


@pytest.mark.parametrize('index,window', [('ivfpq', 'post'), ('ivfflat', 'post'), ('ivfpq', 'pre')])
def test_fused_paths_match_the_filtered_oracle(O, tie, index, window):
    from ann_solo_amd.spectral_library import SpectralLibrary
    nq = 48 if window == 'post' else 32
    q = _queries(tie['lib0'], tie['aux'], nq, seed=73, with_copies=6)
    n = tie['lib'].n
    keep = np.arange(n) % 3 == 0
    keep[:400] = np.arange(400) % 2 == 0
    sl = SpectralLibrary(tie['lib'], config=_config(index, window))
    try:
        before = sl._search_batch(q, 2, 'open', want_knn=True)
        sl.set_search_subset({2: keep})
        res = sl._search_batch(q, 2, 'open', want_knn=True)
        _assert_batch(res, _oracle_batch(O, sl, q, keep, 250.0, per_query_window=window == 'pre'), (index, window))
        assert keep[res.best_row[res.best_row >= 0]].all()
        assert not np.array_equal(res.knn, before.knn)
        plain = sl._search_batch(q, 2, 'open')          # set-mode rows, the window in the scan's finish
        _same_fields(plain, res, 'set mode')
        sl.set_pipeline(True)
        try:
            qd = q.to('cuda:0')
            a_ = sl._search_batch(qd, 2, 'open', device_out=True)
            b_ = sl._search_batch(qd, 2, 'open', device_out=True, want_knn=True)
            sl.synchronize()
        finally:
            sl.set_pipeline(False)
        _same_fields(a_, res, 'pipelined')
        _same_fields(b_, res, 'pipelined, knn')
        assert np.array_equal(b_.knn.cpu().numpy(), res.knn)
        # replace the selection: the results follow; drop it: the results of before, bit for bit
        keep2 = np.random.default_rng(3).random(n) < 0.3
        sl.set_search_subset({2: keep2})
        res2 = sl._search_batch(q, 2, 'open', want_knn=True)
        _assert_batch(res2, _oracle_batch(O, sl, q, keep2, 250.0, per_query_window=window == 'pre'), 'replaced')
        sl.set_search_subset(None)
        after = sl._search_batch(q, 2, 'open', want_knn=True)
        _same_fields(after, before, 'dropped')
        assert np.array_equal(after.knn, before.knn)
        _same_fields(sl._search_batch(q, 2, 'open'), before, 'dropped, set mode')
    finally:
        sl.shutdown()


def _window_rows(O, Q, i, pmz32, keep, tol, mode):
    return np.array([r for r in np.nonzero(keep)[0] if O.precursor_ok(Q.precursor_mz[i], pmz32[r], 2, tol, mode)],
                    np.int64)


@pytest.mark.parametrize('mode,tol,tmode', [('std', 20.0, 'ppm'), ('open', 250.0, 'Da')])
def test_window_only_paths(O, tie, mode, tol, tmode):
    """use_ann = 0 (cascade level 'std', --mode bf) with a pair budget small enough for several tiles."""
    from ann_solo_amd import _lib
    from ann_solo_amd.spectral_library import SpectralLibrary
    q = _queries(tie['lib0'], tie['aux'], 32, seed=74, with_copies=4)
    n = tie['lib'].n
    keep = np.arange(n) % 3 != 1
    keep[:400] = np.arange(400) % 2 == 0
    sl = SpectralLibrary(tie['lib'], config=_config(mode='bf') if mode == 'open' else _config())
    L = _lib.lib()
    try:
        fresh = sl._search_batch(q, 2, mode)
        sl.set_search_subset({2: keep})
        part = sl.partitions[2]
        Lo = O.Spectra(*part.spectra.to('cpu').numpy())
        Q = O.Spectra(*q.numpy())
        whole = sl._search_batch(q, 2, mode)
        total = int(whole.n_candidates.astype(np.int64).sum())
        budget = max(total // 5, 1)
        assert total > 2 * budget                    # several tiles
        prev = L.asl_set_window_pair_budget(budget)
        try:
            tiled = sl._search_batch(q, 2, mode)
            top = sl.search_batch_topn(q, 2, mode, 3)
        finally:
            L.asl_set_window_pair_budget(prev)
        _same_fields(tiled, whole, 'several tiles')
        for f in ('best_row', 'best_score', 'pm_count', 'pm_pairs'):
            assert np.array_equal(getattr(top, f)[:, 0], getattr(whole, f)), f
        assert keep[top.best_row[top.best_row >= 0]].all()
        for i in range(q.n):
            want = _window_rows(O, Q, i, part.precursor_mz, keep, tol, tmode)
            assert whole.n_candidates[i] == len(want), i
            b, s, m = O.best_match(Q, i, Lo, want, 0.02, True)
            if b < 0:
                assert whole.best_row[i] == -1
                continue
            assert whole.best_row[i] == want[b] and whole.best_score[i] == s, i
            assert np.array_equal(whole.peak_matches(i), m), i
        sl.set_search_subset(None)
        _same_fields(sl._search_batch(q, 2, mode), fresh, 'dropped')
    finally:
        sl.shutdown()


def _ranks(O, Q, i, L, cand, n, groups=None):
    """[(row, score, matches)]: O.best_match, the winner deleted, until n ranks (of n different groups)."""
    cand = np.sort(np.asarray(cand, np.int64))      # equal scores: the lower library row
    out, seen = [], set()
    while len(out) < n and len(cand):
        b, s, m = O.best_match(Q, i, L, cand, 0.02, True)
        assert b >= 0
        row = int(cand[b])
        cand = np.delete(cand, b)
        if groups is not None:
            if int(groups[row]) in seen:
                continue
            seen.add(int(groups[row]))
        out.append((row, s, m))
    return out


@pytest.mark.parametrize('index,window', [('ivfpq', 'post'), ('ivfflat', 'post'), ('ivfpq', 'pre')])
def test_ranked_matches_plain_and_distinct(O, tie, index, window):
    """num_matches = 3 over the selected candidates, plain and one rank per group."""
    from ann_solo_amd.spectral_library import SpectralLibrary
    q = _queries(tie['lib0'], tie['aux'], 24, seed=75, with_copies=4)
    n = tie['lib'].n
    keep = np.arange(n) % 3 == 0
    keep[:400] = np.arange(400) % 2 == 0
    groups = (np.arange(n) % 11).astype(np.int32)
    sl = SpectralLibrary(tie['lib'], config=_config(index, window))
    try:
        sl.set_search_subset({2: keep})
        sl.set_match_groups({2: groups})
        single = sl._search_batch(q, 2, 'open', want_knn=True)
        part = sl.partitions[2]
        Lo = O.Spectra(*part.spectra.to('cpu').numpy())
        Q = O.Spectra(*q.numpy())
        q_pmz = q.numpy()[4].astype(np.float64)
        for distinct in (False, True):
            top = sl.search_batch_topn(q, 2, 'open', 3, want_knn=True, distinct=distinct)
            assert np.array_equal(top.knn, single.knn)
            assert np.array_equal(top.n_candidates, single.n_candidates)
            for i in range(q.n):
                ids = single.knn[i][single.knn[i] >= 0]
                assert keep[ids].all()
                cand = ids[_window_mask(q_pmz[i], part.precursor_mz[ids], 2, 250.0, 'Da')]
                want = _ranks(O, Q, i, Lo, cand, 3, groups if distinct else None)
                for r in range(3):
                    if r >= len(want):
                        assert top.best_row[i, r] == -1 and top.best_score[i, r] == 0.0 and top.pm_count[i, r] == 0
                        continue
                    row, s, m = want[r]
                    assert top.best_row[i, r] == row and top.best_score[i, r] == s, (distinct, i, r)
                    assert np.array_equal(top.peak_matches(i, r), m), (distinct, i, r)
            for f in ('best_row', 'best_score', 'pm_count', 'pm_pairs'):
                assert np.array_equal(getattr(top, f)[:, 0], getattr(single, f)), (distinct, f)
    finally:
        sl.shutdown()


def test_rescore_knn_drops_unselected_rows(O, tie):
    """asl_rescore_knn over the ids of a PLAIN search: an unselected row among them is not a candidate."""
    import ctypes as C
    from ann_solo_amd import _lib
    from ann_solo_amd.spectral_library import SpectralLibrary, get_dim, HASH_SEED
    q = _queries(tie['lib0'], tie['aux'], 24, seed=76, with_copies=4)
    n = tie['lib'].n
    keep = np.arange(n) % 3 == 0
    sl = SpectralLibrary(tie['lib'], config=_config())
    try:
        knn = np.ascontiguousarray(sl._search_batch(q, 2, 'open', want_knn=True).knn)
        sl.set_search_subset({2: keep})
        part = sl.partitions[2]
        cfg = sl.config
        _, min_bound, _ = get_dim(cfg.min_mz, cfg.max_mz, cfg.bin_size)
        P = _lib.AslSearchParams(min_bound, cfg.bin_size, HASH_SEED, 256, NPROBE, 2, 250.0, 0,
                                 cfg.fragment_mz_tolerance, int(cfg.allow_peak_shifts), 1)
        row, score = np.empty(q.n, np.int32), np.empty(q.n, np.float64)
        ncand, cnt = np.empty(q.n, np.int32), np.empty(q.n, np.int32)
        pairs = np.empty((q.n, 64, 2), np.uint32)
        _lib.check(_lib.lib().asl_rescore_knn(part.handle, C.byref(_lib.peaks_struct(q)), C.byref(P), _lib.ptr(knn),
                                              _lib.ptr(row), _lib.ptr(score), _lib.ptr(ncand), _lib.ptr(cnt),
                                              _lib.ptr(pairs), 64))
        Lo = O.Spectra(*part.spectra.to('cpu').numpy())
        Q = O.Spectra(*q.numpy())
        q_pmz = q.numpy()[4].astype(np.float64)
        dropped = 0
        for i in range(q.n):
            ids = knn[i][knn[i] >= 0]
            cand = ids[keep[ids] & _window_mask(q_pmz[i], part.precursor_mz[ids], 2, 250.0, 'Da')]
            dropped += int((~keep[ids]).sum())
            assert ncand[i] == len(cand), i
            want = _ranks(O, Q, i, Lo, cand, 1)
            if not want:
                assert row[i] == -1
                continue
            assert row[i] == want[0][0] and score[i] == want[0][1], i
            assert np.array_equal(pairs[i, :cnt[i]].astype(np.int64), want[0][2]), i
        assert dropped > 0
        # the ranked calls over the same ids, plain and one rank per group
        groups = (np.arange(n) % 11).astype(np.int32)
        sl.set_match_groups({2: groups})
        L = _lib.lib()
        for fn, grp in ((L.asl_rescore_knn_topn, None), (L.asl_rescore_knn_topn_distinct, groups)):
            rows, scores = np.empty((q.n, 3), np.int32), np.empty((q.n, 3), np.float64)
            nc, cnts = np.empty(q.n, np.int32), np.empty((q.n, 3), np.int32)
            prs = np.empty((q.n, 3, 64, 2), np.uint32)
            _lib.check(fn(part.handle, C.byref(_lib.peaks_struct(q)), C.byref(P), _lib.ptr(knn), 3, _lib.ptr(rows),
                          _lib.ptr(scores), _lib.ptr(nc), _lib.ptr(cnts), _lib.ptr(prs), 64))
            assert np.array_equal(nc, ncand)
            assert np.array_equal(rows[:, 0], row) and np.array_equal(scores[:, 0], score)
            for i in range(q.n):
                ids = knn[i][knn[i] >= 0]
                cand = ids[keep[ids] & _window_mask(q_pmz[i], part.precursor_mz[ids], 2, 250.0, 'Da')]
                want = _ranks(O, Q, i, Lo, cand, 3, grp)
                for r in range(3):
                    if r >= len(want):
                        assert rows[i, r] == -1 and scores[i, r] == 0.0 and cnts[i, r] == 0, (i, r)
                        continue
                    assert rows[i, r] == want[r][0] and scores[i, r] == want[r][1], (grp is not None, i, r)
                    assert np.array_equal(prs[i, r, :cnts[i, r]].astype(np.int64), want[r][2]), (i, r)
            assert keep[rows[rows >= 0]].all()
    finally:
        sl.shutdown()


# ------------------------------------------------------------------ lifecycle

def test_masks_follow_the_library_handle(O, tie):
    """An index searched with library A and its subset, then -- same index handle -- with library B
    created after A was freed (same size, another subset): the selector words are B's."""
    from ann_solo_amd.spectral_library import SpectralLibrary
    q = _queries(tie['lib0'], tie['aux'], 32, seed=77, with_copies=4)
    n = tie['lib'].n
    keepA, keepB = np.arange(n) % 3 == 0, np.arange(n) % 3 == 1
    slA = SpectralLibrary(tie['lib'], config=_config())
    slA.set_search_subset({2: keepA})
    resA = slA._search_batch(q, 2, 'open', want_knn=True)
    idx = slA.partitions[2].index
    slA.partitions[2].index = None
    slA.shutdown()
    slB = SpectralLibrary(tie['lib'], config=_config())
    try:
        slB.partitions[2].index = idx
        slB.set_search_subset({2: keepB})
        resB = slB._search_batch(q, 2, 'open', want_knn=True)
        assert not np.array_equal(resA.knn, resB.knn)
        _assert_batch(resB, _oracle_batch(O, slB, q, keepB, 250.0), 'library B')
        _same_fields(slB._search_batch(q, 2, 'open'), resB, 'library B, set mode')
    finally:
        slB.shutdown()


def test_dropping_equals_a_fresh_handle(tie):
    from ann_solo_amd.spectral_library import SpectralLibrary
    q = _queries(tie['lib0'], tie['aux'], 32, seed=78, with_copies=4)
    n = tie['lib'].n
    out = []
    for use in (False, True):
        sl = SpectralLibrary(tie['lib'], config=_config())
        try:
            if use:
                sl.set_search_subset({2: np.arange(n) % 5 == 0})
                assert (sl._search_batch(q, 2, 'open').n_candidates >= 0).all()
                sl._search_batch(q, 2, 'std')
                sl.set_search_subset(None)
            out.append((sl._search_batch(q, 2, 'open', want_knn=True), sl._search_batch(q, 2, 'open'),
                        sl._search_batch(q, 2, 'std')))
        finally:
            sl.shutdown()
    for a, b in zip(*out):
        _same_fields(a, b)
    assert np.array_equal(out[0][0].knn, out[1][0].knn)


@pytest.mark.parametrize('kind', ['pq', 'flat'])
def test_add_drops_the_selector(O, tie, kind):
    xb, xq = tie['xb'], tie['xq']
    idx = _new_index(kind, xb[:3000])
    keep = np.arange(3000) % 2 == 0
    idx.set_selector(keep)
    assert (idx.search_selected(xq, 32)[1] % 2 == 0).all()
    idx.add(xb[3000:3500])
    with pytest.raises(Exception, match=ERR_STATE):
        idx.search_selected(xq, 32)
    keep = np.arange(3500) % 2 == 1
    idx.set_selector(keep)
    R.assert_rows_equal(idx.search_selected(xq, 32), R.search_selected(O, R.host_ivf(O, idx), xq, 32, NPROBE, keep))


# ------------------------------------------------------------------ what is not supported is an error

def _rc_selected(L, idx, xq, k):
    from ann_solo_amd import _lib
    D, I = np.empty((len(xq), k), np.float32), np.empty((len(xq), k), np.int64)
    return L.asl_index_search_selected(idx._h, len(xq), _lib.ptr(xq), None, 0, 0.0, 0, k, int(idx.nprobe),
                                       _lib.ptr(D), _lib.ptr(I))


def test_unsupported_cases_are_errors(tie):
    from ann_solo_amd import _lib, faiss_compat as faiss
    from ann_solo_amd.spectral_library import SpectralLibrary
    L = _lib.lib()
    STATE, INVALID = -3, -1
    xb, xq = tie['xb'][:3000], np.ascontiguousarray(tie['xq'][:8])
    keep = np.ascontiguousarray((np.arange(3000) % 2 == 0).astype(np.uint8))
    for kind in ('pq', 'flat'):
        idx = _new_index(kind, xb, nlist=8, niter=2)
        assert L.asl_index_set_selector(idx._h, 2999, _lib.ptr(keep)) == INVALID     # a wrong n
        assert _rc_selected(L, idx, xq, 16) == STATE                                  # no selector yet
        idx.set_selector(keep)
        assert _rc_selected(L, idx, xq, 16) == 0
        assert _rc_selected(L, idx, xq, 1280) == 0
        assert _rc_selected(L, idx, xq, 1281) == STATE                                # k > 1280
        idx.set_scan_variant(1)                                                       # the generic kernels
        assert _rc_selected(L, idx, xq, 16) == STATE
        assert b'scan_variant' in L.asl_last_error()
        idx.set_scan_variant(0)
        idx.set_unordered(2)                                                          # packed-key rows
        assert _rc_selected(L, idx, xq, 16) == STATE
        idx.set_unordered(0)
        assert _rc_selected(L, idx, xq, 16) == 0
        idx.shard(0, 2)                                                               # a sharded index
        assert _rc_selected(L, idx, xq, 16) == STATE
        idx.set_selector(keep)
        assert _rc_selected(L, idx, xq, 16) == STATE and b'sharded' in L.asl_last_error()
    # another PQ shape (the generic kernel serves it)
    pq16 = _new_index('pq', xb, nlist=8, niter=2, m=16)
    pq16.set_selector(keep)
    assert _rc_selected(L, pq16, xq, 16) == STATE and b'tiled' in L.asl_last_error()
    # the exact re-rank
    ref = faiss.IndexIVFPQ(faiss.IndexFlatIP(800), 800, 8, 32, 8)
    ref.set_niter(2)
    ref.set_refine(256)
    ref.train(xb)
    ref.add(xb)
    ref.nprobe = 4
    ref.set_selector(keep)
    assert _rc_selected(L, ref, xq, 16) == STATE and b're-rank' in L.asl_last_error()
    # dense rows (no postings) and a Flat index
    rng = np.random.default_rng(4)
    xd = rng.random((2000, 64), dtype=np.float32)
    xd /= np.linalg.norm(xd, axis=1, keepdims=True)
    dense = faiss.IndexIVFFlat(faiss.IndexFlatIP(64), 64, 8)
    dense.set_niter(2)
    dense.train(xd)
    dense.add(xd)
    dense.nprobe = 4
    assert dense.flat_layout == 0
    dense.set_selector(np.ones(2000, bool))
    assert _rc_selected(L, dense, xd[:8].copy(), 16) == STATE and b'dense' in L.asl_last_error()
    flat = faiss.IndexFlatIP(64)
    flat.add(xd)
    flat.set_selector(np.ones(2000, bool))
    assert _rc_selected(L, flat, xd[:8].copy(), 16) == STATE and b'Flat' in L.asl_last_error()
    # the fused calls return the index's error, and a wrong n is refused
    q = _queries(tie['lib0'], tie['aux'], 16, seed=79)
    sl = SpectralLibrary(tie['lib'], config=_config())
    try:
        part = sl.partitions[2]
        wrong = np.ones(tie['lib'].n - 1, np.uint8)
        assert L.asl_library_set_selection(part.handle, len(wrong), _lib.ptr(wrong)) == INVALID
        sl._get_ann_index(2).set_scan_variant(1)
        sl._search_batch(q, 2, 'open')                       # no selection: the generic kernels serve it
        sl.set_search_subset({2: np.arange(tie['lib'].n) % 2 == 0})
        with pytest.raises(_lib.AnnSoloMiError, match=ERR_STATE):
            sl._search_batch(q, 2, 'open')
        with pytest.raises(_lib.AnnSoloMiError, match=ERR_STATE):
            sl.search_batch_topn(q, 2, 'open', 3)
        sl._search_batch(q, 2, 'std')                        # the window-only level needs no index
    finally:
        sl.shutdown()
