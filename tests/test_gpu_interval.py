"""Per-query precursor intervals (ASL_TOL_INTERVAL; ``mode='interval'``, ``windows=``): every site that
applies the precursor window, against the unchanged oracle run on a key column masked per query
(tests/interval_ref.py) -- ids, score bits, winners, scores, candidate counts, peak matches and neighbour
rows equal, no tolerance. Shapes: the 5 000-spectrum tie library of the window-scan tests (rows 0 .. 399 are
copies of one spectrum: ties at the k-th score), nlist 16, nprobe 8, k = 256 (64 and 1 024 once each), 48
queries of which the first 8 are copies of row 0."""
import ctypes as C

import numpy as np
import pytest

import interval_ref as R

pytestmark = pytest.mark.gpu

FIELDS = ('best_row', 'best_score', 'n_candidates', 'pm_count', 'pm_pairs')
NLIST, NPROBE, K, NQ, COPIES = 16, 8, 256, 48, 8
CASES = ('m50_p250', 'p10_p250', 'm250_m10', 'iso4', 'one_row', 'empty', 'all', 'nan_some')
ERR_INVALID, ERR_STATE = 'error -1', 'error -3'


class World:
    def __init__(self, O):
        self.O = O
        self.lib0, self.aux, self.lib = R.tie_library()
        self.q = R.tie_queries(self.lib0, self.aux, NQ, seed=72, with_copies=COPIES)
        self.Q = O.Spectra(*self.q.numpy())
        self.q_pmz = self.q.numpy()[4].astype(np.float64)
        self.sl, self.ivf, self.refs = {}, {}, {}
        self.key0 = None

    def library(self, kind):
        """kind: 'pq' | 'flat' | 'fx22' (post order) | 'pre' (IVF-PQ, window scan)."""
        from ann_solo_amd.spectral_library import Config, SpectralLibrary
        if kind not in self.sl:
            kw = dict(index='ivfflat', flat_storage='fx22' if kind == 'fx22' else 'fp32') if kind in ('flat', 'fx22') \
                else dict(index='ivfpq', ann_window='pre' if kind == 'pre' else 'post')
            cfg = Config.open_search(num_list=NLIST, num_probe=NPROBE, num_candidates=K, kmeans_niter=4,
                                     precursor_tolerance_mass_open=250.0, precursor_tolerance_mode_open='Da', **kw)
            sl = self.sl[kind] = SpectralLibrary(self.lib, config=cfg)
            self.ivf[kind] = R.host_ivf(self.O, sl._get_ann_index(2))
            if self.key0 is None:
                part = sl.partitions[2]
                self.key0 = np.ascontiguousarray(part.precursor_mz, np.float32)
                self.L = self.O.Spectra(*part.spectra.to('cpu').numpy())
                self.wins, self.one_rows = R.window_cases(self.q_pmz, self.key0, COPIES)
                self.xq = sl._encode(self.q.to(sl.device)).cpu().numpy()
        return self.sl[kind], self.ivf[kind]

    def reference(self, kind, case, keep=None):
        """The oracle's batch for one index kind and window case (keep: a selection, by row)."""
        tag = (kind, case, None if keep is None else keep.tobytes())
        if tag not in self.refs:
            _, ivf = self.library(kind)
            key = self.key0 if keep is None else np.where(keep, self.key0, np.float32(np.nan)).astype(np.float32)
            if keep is not None:
                ivf = R.filtered(self.O, ivf, keep)
            self.refs[tag] = R.oracle_batch(self.O, self.q, self.L, ivf, key, self.wins[case], K, NPROBE,
                                            'pre' if kind == 'pre' else 'post')
        return self.refs[tag]

    def close(self):
        for sl in self.sl.values():
            sl.shutdown()


@pytest.fixture(scope='module')
def world(O):
    w = World(O)
    yield w
    w.close()


def _np(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


def _assert_batch(res, ref, what=''):
    if res.knn is not None:
        assert np.array_equal(_np(res.knn), ref['knn_I']), what
    for f, g in (('n_candidates', 'n_cand'), ('best_row', 'best_row'), ('best_score', 'best_score'),
                 ('pm_count', 'pm_count')):
        assert np.array_equal(_np(getattr(res, f)), ref[g]), (what, f)
    cnt, pairs = _np(res.pm_count), _np(res.pm_pairs)
    for i in range(len(cnt)):
        assert np.array_equal(pairs[i, :cnt[i]].astype(np.uint32), ref['pm_pairs'][i, :cnt[i]]), (what, i)


def _same_fields(a, b, what=''):
    for f in FIELDS:
        x, y = _np(getattr(a, f)), _np(getattr(b, f))
        assert np.array_equal(x.astype(y.dtype), y), (what, f)


# ------------------------------------------------------------------ index level
def test_index_level_search_window(O, world):
    """asl_index_search_window with mode 2 (refused before the interval mode existed)."""
    sl, ivf = world.library('pq')
    idx = sl._get_ann_index(2)
    xq, key0, q_pmz = world.xq, world.key0, world.q_pmz
    key_nan = key0.copy()
    key_nan[::7] = np.nan
    idx.nprobe = NPROBE
    short = 0
    todo = [(key0, c, K) for c in CASES] + [(key_nan, 'm50_p250', K), (key_nan, 'all', K), (key0, 'm50_p250', 64),
                                            (key0, 'm50_p250', 1024)]
    for key, case, k in todo:
        w = world.wins[case]
        idx.set_window_key(key)
        D, I = idx.search_window(xq, k, w, 2, 0.0, 'interval')
        print('search_window', case, k, 'nan key' if key is key_nan else '', 'hits', int((I >= 0).sum()),
              'short rows', int((I < 0).any(1).sum()))
        R.assert_rows_equal((D, I), R.index_rows(O, ivf, xq, k, NPROBE, key, w), (case, k))
        for i in range(NQ):
            hit = I[i][I[i] >= 0]
            assert R.interval_mask(key[hit], w[i, 0], w[i, 1]).all(), (case, k, i)
        short += int((I < 0).any(1).sum()) if case == 'm50_p250' and k == K else 0
        if case == 'empty':
            assert (I == -1).all()
        if case == 'one_row' and key is key0:         # the one row, where its list is probed
            assert ((I[:, 0] == world.one_rows) | (I[:, 0] == -1)).all() and (I[:, 1:] == -1).all()
            assert (I[:, 0] >= 0).any()
        if case == 'nan_some':
            assert (I[np.isnan(w).any(1)] == -1).all() and (I[~np.isnan(w).any(1), 0] >= 0).any()
        if case == 'all':                             # the bytes of the Da mode with tol = 1e9
            D2, I2 = idx.search_window(xq, k, q_pmz, 2, 1e9, 'Da')
            assert np.array_equal(I, I2) and np.array_equal(D.view(np.uint32), D2.view(np.uint32))
    assert short > 0
    idx.set_window_key(key0)
    # ties at the k-th score: the copies of row 0 fill the rows of the first queries beyond k
    _, I = idx.search_window(xq[:COPIES], 64, world.wins['m50_p250'][:COPIES], 2, 0.0, 'interval')
    assert (I < 400).all() and (I >= 0).all()
    # the dyadic case: q on multiples of 0.5, +-128 m/z is +-256 Da at charge 2, exactly
    qd = np.round(q_pmz * 2.0) / 2.0
    Dd, Id = idx.search_window(xq, K, np.stack([qd - 128.0, qd + 128.0], 1), 2, 0.0, 'interval')
    D2, I2 = idx.search_window(xq, K, qd, 2, 256.0, 'Da')
    assert np.array_equal(Id, I2) and np.array_equal(Dd.view(np.uint32), D2.view(np.uint32)) and (Id[:, 0] >= 0).all()
    # device tensors stay on the device
    import torch
    w = world.wins['m50_p250']
    Dt, It = idx.search_window(torch.as_tensor(xq, device='cuda:0'), K, torch.as_tensor(w, device='cuda:0'), 2, 0.0,
                               'interval')
    Dh, Ih = idx.search_window(xq, K, w, 2, 0.0, 'interval')
    assert np.array_equal(It.cpu().numpy(), Ih) and np.array_equal(Dt.cpu().numpy().view(np.uint32), Dh.view(np.uint32))


def test_index_level_search_selected_with_a_window(O, world):
    sl, ivf = world.library('pq')
    idx = sl._get_ann_index(2)
    idx.nprobe = NPROBE
    key0 = world.key0
    key_nan = key0.copy()
    key_nan[::7] = np.nan
    keep = np.arange(len(key0)) % 2 == 0
    idx.set_selector(keep)
    try:
        for key, case in ((key0, 'm50_p250'), (key0, 'iso4'), (key0, 'empty'), (key0, 'nan_some'), (key_nan, 'p10_p250')):
            idx.set_window_key(key)
            w = world.wins[case]
            got = idx.search_selected(world.xq, K, window=(w, 2, 0.0, 'interval'))
            sel_key = np.where(keep, key, np.float32(np.nan)).astype(np.float32)
            R.assert_rows_equal(got, R.index_rows(O, ivf, world.xq, K, NPROBE, sel_key, w), case)
            hit = got[1][got[1] >= 0]
            assert keep[hit].all()
    finally:
        idx.set_selector(None)
        idx.set_window_key(key0)
    # IVF-Flat has no window-ordered layout: refused in interval mode as in Da mode, with the same message
    fsl, _ = world.library('flat')
    flat = fsl._get_ann_index(2)
    flat.set_selector(keep)
    msgs = []
    for win in ((world.q_pmz, 2, 250.0, 'Da'), (world.wins['m50_p250'], 2, 0.0, 'interval')):
        with pytest.raises(Exception, match=ERR_STATE) as e:
            flat.search_selected(world.xq, K, window=win)
        msgs.append(str(e.value))
    flat.set_selector(None)
    assert msgs[0] == msgs[1]


@pytest.mark.parametrize('kind', ['pq', 'flat'])
def test_rank_of_with_a_key(O, world, kind):
    from rank_ref import expected_ranks
    sl, ivf = world.library(kind)
    idx = sl._get_ann_index(2)
    key0, xq = world.key0, world.xq
    key_nan = key0.copy()
    key_nan[::7] = np.nan
    n = len(key0)
    inside = 0
    for key, case in ((key0, 'm50_p250'), (key0, 'p10_p250'), (key0, 'one_row'), (key0, 'empty'), (key0, 'nan_some'),
                      (key_nan, 'm50_p250')):
        w = world.wins[case]
        rD, rI = R.index_rows(O, ivf, xq, n, NPROBE, key, w)          # the whole scope, in neighbour order
        # targets: a hit in the middle of the scope, the one row, a row outside the window, -1
        T = np.array([rI[i, (rI[i] >= 0).sum() // 2] for i in range(NQ)], np.int64)
        T[1::4] = world.one_rows[1::4]
        T[2::8] = -1
        rank, score, scope = idx.rank_of(xq, T, NPROBE, (key, w, 2, 0.0, 'interval'))
        want = expected_ranks(rI, T)
        print('rank_of', kind, case, 'in scope', int((want >= 0).sum()), 'max rank', int(want.max()), 'scope',
              int(scope.sum()))
        assert np.array_equal(rank, want), (kind, case)
        assert np.array_equal(scope, (rI >= 0).sum(1)), (kind, case)
        hit = want >= 0
        assert np.array_equal(score.view(np.uint32)[hit], rD[np.nonzero(hit)[0], want[hit]].view(np.uint32)), (kind, case)
        assert np.isnan(score[~hit]).all()
        inside += int(hit.sum())
        if case == 'empty':
            assert (rank == -1).all() and (scope == 0).all()
    assert inside > NQ
    # (-inf, +inf): the Da mode with tol = 1e9
    T = np.arange(NQ, dtype=np.int64) * 7
    a = idx.rank_of(xq, T, NPROBE, (key0, world.wins['all'], 2, 0.0, 'interval'))
    b = idx.rank_of(xq, T, NPROBE, (key0, world.q_pmz, 2, 1e9, 'Da'))
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


# ------------------------------------------------------------------ fused paths
@pytest.mark.parametrize('kind', ['pq', 'flat', 'fx22', 'pre'])
def test_fused_paths_match_the_oracle(O, world, kind):
    """use_ann = 1: with the neighbour list (the rescoring filters), as a set with the scan-side post-filter
    on and off, pipelined; 'pre' is the window scan."""
    from ann_solo_amd import _lib
    sl, _ = world.library(kind)
    q = world.q
    L = _lib.lib()
    before = sl._search_batch(q, 2, 'open', want_knn=True)
    diff = short = 0
    for case in CASES:
        w = world.wins[case]
        ref = world.reference(kind, case)
        res = sl._search_batch(q, 2, 'open', want_knn=True, windows=w)
        print('fused', kind, case, 'candidates', int(res.n_candidates.sum()), 'oracle', int(ref['n_cand'].sum()),
              'matched queries', int((res.best_row >= 0).sum()), 'differ from +-250 Da',
              int((res.n_candidates != before.n_candidates).sum()))
        _assert_batch(res, ref, (kind, case, 'knn'))
        for pf in (1, 0):
            prev = L.asl_set_scan_postfilter(pf)
            try:
                plain = sl._search_batch(q, 2, 'open', windows=w)
            finally:
                L.asl_set_scan_postfilter(prev)
            _same_fields(plain, res, (kind, case, 'set mode, post-filter %d' % pf))
        if case == 'm50_p250':
            diff = int((res.n_candidates != before.n_candidates).sum())
            short = int((res.knn < 0).any(1).sum())
        if case == 'empty':
            assert (res.best_row == -1).all() and (res.n_candidates == 0).all()
        if case == 'p10_p250':                        # the unmodified match is outside
            assert not np.array_equal(res.best_row, before.best_row)
    assert diff >= NQ // 2
    assert short > 0 or kind != 'pre'
    # pipelined: two batches in flight, different windows
    import torch
    sl.set_pipeline(True)
    try:
        qd = q.to('cuda:0')
        a_ = sl._search_batch(qd, 2, 'open', device_out=True, windows=world.wins['m50_p250'])
        b_ = sl._search_batch(qd, 2, 'open', device_out=True, want_knn=True,
                              windows=torch.as_tensor(world.wins['nan_some'], device='cuda:0'))
        c_ = sl._search_batch(qd, 2, 'open', device_out=True, windows=world.wins['iso4'])
        sl.synchronize()
    finally:
        sl.set_pipeline(False)
    _assert_batch(a_, world.reference(kind, 'm50_p250'), (kind, 'pipelined'))
    _assert_batch(b_, world.reference(kind, 'nan_some'), (kind, 'pipelined, knn'))
    _assert_batch(c_, world.reference(kind, 'iso4'), (kind, 'pipelined'))
    # dropping windows= again: the bytes of before
    after = sl._search_batch(q, 2, 'open', want_knn=True)
    _same_fields(after, before, 'dropped')
    assert np.array_equal(after.knn, before.knn)
    _same_fields(sl._search_batch(q, 2, 'open'), before, 'dropped, set mode')


@pytest.mark.parametrize('kind', ['pq', 'flat', 'pre'])
def test_identities_with_the_da_mode(world, kind):
    from ann_solo_amd.packed import PackedSpectra
    sl, _ = world.library(kind)
    q = world.q
    cfg = sl.config
    old = cfg.precursor_tolerance_mass_open
    try:
        cfg.precursor_tolerance_mass_open = 1e9       # (-inf, +inf) is the Da mode with tol = 1e9
        for knn in (True, False):
            a = sl._search_batch(q, 2, 'open', want_knn=knn)
            b = sl._search_batch(q, 2, 'open', want_knn=knn, windows=world.wins['all'])
            _same_fields(b, a, (kind, 'all', knn))
            assert not knn or np.array_equal(a.knn, b.knn)
        # the dyadic case: charge 2, tol 256 Da, query precursors on multiples of 0.5
        o, mz, it, chg, pmz, pz = q.numpy()
        qd = np.round(np.asarray(pmz, np.float64) * 2.0) / 2.0
        qdy = PackedSpectra.from_numpy(o, mz, it, chg, qd, pz)
        cfg.precursor_tolerance_mass_open = 256.0
        wd = np.stack([qd - 128.0, qd + 128.0], 1)
        for knn in (True, False):
            a = sl._search_batch(qdy, 2, 'open', want_knn=knn)
            b = sl._search_batch(qdy, 2, 'open', want_knn=knn, windows=wd)
            _same_fields(b, a, (kind, 'dyadic', knn))
            assert not knn or np.array_equal(a.knn, b.knn)
        assert (a.n_candidates > 0).any()
        # use_ann = 0 (the standard level's window walk) at the same tolerance
        std = cfg.precursor_tolerance_mass, cfg.precursor_tolerance_mode
        cfg.precursor_tolerance_mass, cfg.precursor_tolerance_mode = 256.0, 'Da'
        try:
            _same_fields(sl._search_batch(qdy, 2, 'std', windows=wd), sl._search_batch(qdy, 2, 'std'), (kind, 'bf'))
        finally:
            cfg.precursor_tolerance_mass, cfg.precursor_tolerance_mode = std
    finally:
        cfg.precursor_tolerance_mass_open = old


def _check_ranks(top, i, ranks, n, what):
    for r in range(n):
        if r < len(ranks):
            row, s, m = ranks[r]
            assert top.best_row[i, r] == row and top.best_score[i, r] == s, (what, i, r)
            assert np.array_equal(top.peak_matches(i, r), m), (what, i, r)
        else:
            assert top.best_row[i, r] == -1 and top.best_score[i, r] == 0.0 and top.pm_count[i, r] == 0, (what, i, r)


def test_window_only_search_in_one_tile_and_in_many(O, world):
    """use_ann = 0 (the standard level's walk, --mode bf) with windows=: n_candidates, winner, score and peak
    matches against the oracle's best match over the window's rows; tiles of a few thousand pairs; top-n."""
    from ann_solo_amd import _lib
    sl, _ = world.library('pq')
    q, key, Q, Lo = world.q, world.key0, world.Q, world.L
    L = _lib.lib()
    groups = (np.arange(len(key)) // 3).astype(np.int32)
    sl.set_match_groups({2: groups})
    for case in ('m50_p250', 'm250_m10', 'one_row', 'empty', 'nan_some', 'all'):
        w = world.wins[case]
        whole = sl._search_batch(q, 2, 'std', windows=w)
        total = int(whole.n_candidates.astype(np.int64).sum())
        cands = [R.window_rows(key, w, i) for i in range(NQ)]
        print('window only', case, 'pairs', total, 'oracle', sum(len(c) for c in cands))
        assert np.array_equal(whole.n_candidates, [len(c) for c in cands]), case
        lists = sl._get_library_candidates(q, 2, 'std', windows=w)
        for i in range(NQ):
            assert np.array_equal(lists[i], cands[i]), (case, i)
        for i in range(0, NQ, 1 if case != 'all' else 6):
            b, s, m = O.best_match(Q, i, Lo, cands[i], R.FRAG_TOL, True)
            if b < 0:
                assert whole.best_row[i] == -1, (case, i)
                continue
            assert whole.best_row[i] == cands[i][b] and whole.best_score[i] == s, (case, i)
            assert np.array_equal(whole.peak_matches(i), m), (case, i)
        if total == 0:
            assert (whole.best_row == -1).all()
            continue
        budget = min(max(total // 5, 1), 4000)
        prev = L.asl_set_window_pair_budget(budget)
        try:
            tiled = sl._search_batch(q, 2, 'std', windows=w)
            top = sl.search_batch_topn(q, 2, 'std', 5, windows=w)
            dis = sl.search_batch_topn(q, 2, 'std', 5, distinct=True, windows=w)
        finally:
            L.asl_set_window_pair_budget(prev)
        assert total > 2 * budget                                # several tiles
        _same_fields(tiled, whole, (case, 'tiled'))
        if case in ('m50_p250', 'one_row'):
            for i in range(0, NQ, 5):
                _check_ranks(top, i, R.oracle_ranks(O, Q, i, Lo, cands[i], 5), 5, (case, 'topn'))
                _check_ranks(dis, i, R.oracle_ranks(O, Q, i, Lo, cands[i], 5, groups), 5, (case, 'distinct'))
        for f in ('best_row', 'best_score', 'pm_count', 'pm_pairs'):
            assert np.array_equal(getattr(top, f)[:, 0], getattr(whole, f)), (case, f)
    sl.set_match_groups(None)


@pytest.mark.parametrize('kind', ['pq', 'flat', 'pre'])
def test_topn_and_distinct_ranks(O, world, kind):
    sl, _ = world.library(kind)
    q, key, Q, Lo = world.q, world.key0, world.Q, world.L
    groups = (np.arange(len(key)) // 3).astype(np.int32)
    sl.set_match_groups({2: groups})
    try:
        for case in ('m50_p250', 'p10_p250', 'nan_some'):
            w = world.wins[case]
            ref = world.reference(kind, case)
            top = sl.search_batch_topn(q, 2, 'open', 5, want_knn=True, windows=w)
            dis = sl.search_batch_topn(q, 2, 'open', 5, want_knn=True, distinct=True, windows=w)
            for t in (top, dis):
                assert np.array_equal(t.knn, ref['knn_I']) and np.array_equal(t.n_candidates, ref['n_cand'])
                _assert_batch(t.rank0(), ref, (kind, case, 'rank 0'))
            for i in range(0, NQ, 3):
                ids = ref['knn_I'][i][ref['knn_I'][i] >= 0]
                cand = ids[R.interval_mask(key[ids], w[i, 0], w[i, 1])]
                assert len(cand) == ref['n_cand'][i]
                _check_ranks(top, i, R.oracle_ranks(O, Q, i, Lo, cand, 5), 5, (kind, case, 'topn'))
                _check_ranks(dis, i, R.oracle_ranks(O, Q, i, Lo, cand, 5, groups), 5, (kind, case, 'distinct'))
    finally:
        sl.set_match_groups(None)


@pytest.mark.parametrize('kind', ['pq', 'flat', 'pre'])
def test_with_a_selection_installed(O, world, kind):
    sl, _ = world.library(kind)
    q = world.q
    n = len(world.key0)
    keep = np.arange(n) % 2 == 0
    keep[:400] = np.arange(400) % 4 < 2
    before = sl._search_batch(q, 2, 'open', want_knn=True, windows=world.wins['m50_p250'])
    sl.set_search_subset({2: keep})
    try:
        for case in ('m50_p250', 'iso4', 'nan_some'):
            w = world.wins[case]
            ref = world.reference(kind, case, keep)
            res = sl._search_batch(q, 2, 'open', want_knn=True, windows=w)
            _assert_batch(res, ref, (kind, case, 'selection'))
            assert keep[res.best_row[res.best_row >= 0]].all()
            _same_fields(sl._search_batch(q, 2, 'open', windows=w), res, (kind, case, 'selection, set mode'))
            # use_ann = 0: the selected rows of the window
            bf = sl._search_batch(q, 2, 'std', windows=w)
            sel_key = np.where(keep, world.key0, np.float32(np.nan)).astype(np.float32)
            cands = [R.window_rows(sel_key, w, i) for i in range(NQ)]
            assert np.array_equal(bf.n_candidates, [len(c) for c in cands]), (kind, case)
            for i in range(0, NQ, 4):
                b, s, m = O.best_match(world.Q, i, world.L, cands[i], R.FRAG_TOL, True)
                assert bf.best_row[i] == (cands[i][b] if b >= 0 else -1), (kind, case, i)
                assert b < 0 or (bf.best_score[i] == s and np.array_equal(bf.peak_matches(i), m)), (kind, case, i)
    finally:
        sl.set_search_subset(None)
    after = sl._search_batch(q, 2, 'open', want_knn=True, windows=world.wins['m50_p250'])
    _same_fields(after, before, 'selection dropped')
    assert np.array_equal(after.knn, before.knn)


# ------------------------------------------------------------------ the C ABI: rescore_knn, host arrays, errors
def _params(sl, mode_code, window, use_ann=1, tol=250.0):
    from ann_solo_amd import _lib
    from ann_solo_amd.spectrum import HASH_SEED, get_dim
    cfg = sl.config
    _, min_bound, _ = get_dim(cfg.min_mz, cfg.max_mz, cfg.bin_size)
    P = _lib.AslSearchParams(min_bound, cfg.bin_size, HASH_SEED, K, NPROBE, 2, tol, mode_code,
                             cfg.fragment_mz_tolerance, 1, use_ann)
    P.precursor_window = _lib.ptr(window)
    return P


def test_rescore_knn_and_host_arrays(O, world):
    """asl_rescore_knn / _topn honour the member; a host array of intervals is staged, by a pipelined
    asl_search_batch too (its copy is taken before the call returns)."""
    import torch
    from ann_solo_amd import _lib
    sl, _ = world.library('pq')
    L = _lib.lib()
    q = world.q
    part = sl.partitions[2]
    idx = sl._get_ann_index(2)
    stride = 64
    for case in ('m50_p250', 'nan_some'):
        ref = world.reference('pq', case)
        w = np.ascontiguousarray(world.wins[case])
        knn = np.ascontiguousarray(ref['knn_I'])
        row, sc, nc, cnt = (np.empty(NQ, np.int32), np.empty(NQ, np.float64), np.empty(NQ, np.int32),
                            np.empty(NQ, np.int32))
        pairs = np.empty((NQ, stride, 2), np.uint32)
        qs = _lib.peaks_struct(q)
        for win in (w, torch.as_tensor(w, device='cuda:0')):           # host, device
            P = _params(sl, 2, win)
            _lib.check(L.asl_rescore_knn(part.handle, C.byref(qs), C.byref(P), _lib.ptr(knn), _lib.ptr(row),
                                         _lib.ptr(sc), _lib.ptr(nc), _lib.ptr(cnt), _lib.ptr(pairs), stride))
            assert np.array_equal(row, ref['best_row']) and np.array_equal(sc, ref['best_score'])
            assert np.array_equal(nc, ref['n_cand']) and np.array_equal(cnt, ref['pm_count'])
        row5, sc5, cnt5 = np.empty((NQ, 5), np.int32), np.empty((NQ, 5), np.float64), np.empty((NQ, 5), np.int32)
        P = _params(sl, 2, w)
        _lib.check(L.asl_rescore_knn_topn(part.handle, C.byref(qs), C.byref(P), _lib.ptr(knn), 5, _lib.ptr(row5),
                                          _lib.ptr(sc5), _lib.ptr(nc), _lib.ptr(cnt5), None, 0))
        assert np.array_equal(row5[:, 0], ref['best_row']) and np.array_equal(sc5[:, 0], ref['best_score'])
        # asl_search_batch with a HOST array of intervals: synchronous, then pipelined with the array overwritten
        # as soon as the call has returned
        qd = q.to('cuda:0').contiguous()
        qsd = _lib.peaks_struct(qd)
        out = [dict(row=torch.empty(NQ, dtype=torch.int32, device='cuda:0'),
                    sc=torch.empty(NQ, dtype=torch.float64, device='cuda:0'),
                    nc=torch.empty(NQ, dtype=torch.int32, device='cuda:0'),
                    cnt=torch.empty(NQ, dtype=torch.int32, device='cuda:0'),
                    pairs=torch.empty((NQ, stride, 2), dtype=torch.int32, device='cuda:0')) for _ in range(3)]

        def call(o, win):
            P = _params(sl, 2, win)
            _lib.check(L.asl_search_batch(part.handle, idx._h, C.byref(qsd), C.byref(P), _lib.ptr(o['row']),
                                          _lib.ptr(o['sc']), _lib.ptr(o['nc']), _lib.ptr(o['cnt']),
                                          _lib.ptr(o['pairs']), stride, None))
        call(out[0], w)
        sl.set_pipeline(True)
        try:
            for o in out[1:]:
                scratch = w.copy()
                call(o, scratch)
                scratch[:] = np.nan                                    # the caller's array is the caller's again
            sl.synchronize()
        finally:
            sl.set_pipeline(False)
        for o in out:
            assert np.array_equal(o['row'].cpu().numpy(), ref['best_row']), case
            assert np.array_equal(o['sc'].cpu().numpy(), ref['best_score']), case
            assert np.array_equal(o['nc'].cpu().numpy(), ref['n_cand']), case
            assert np.array_equal(o['cnt'].cpu().numpy(), ref['pm_count']), case


def test_errors(world):
    from ann_solo_amd import _lib, faiss_compat as faiss
    sl, _ = world.library('pq')
    L = _lib.lib()
    idx = sl._get_ann_index(2)
    xq, key0, q_pmz, w = world.xq, world.key0, world.q_pmz, np.ascontiguousarray(world.wins['m50_p250'])
    idx.set_window_key(key0)
    D, I = np.empty((NQ, K), np.float32), np.empty((NQ, K), np.int64)
    # mode 3 is still ASL_ERR_INVALID
    assert L.asl_index_search_window(idx._h, NQ, _lib.ptr(xq), _lib.ptr(w), 2, 0.0, 3, K, NPROBE, _lib.ptr(D),
                                     _lib.ptr(I)) == -1
    assert b'mode' in L.asl_last_error()
    idx.set_selector(np.ones(len(key0), bool))
    assert L.asl_index_search_selected(idx._h, NQ, _lib.ptr(xq), _lib.ptr(w), 2, 0.0, 3, K, NPROBE, _lib.ptr(D),
                                       _lib.ptr(I)) == -1
    idx.set_selector(None)
    T, rank = np.zeros(NQ, np.int64), np.empty(NQ, np.int64)
    assert L.asl_index_rank(idx._h, NQ, _lib.ptr(xq), _lib.ptr(T), NPROBE, _lib.ptr(key0), _lib.ptr(w), 2, 0.0, 3,
                            _lib.ptr(rank), None, None) == -1
    assert L.asl_index_search_window(idx._h, NQ, _lib.ptr(xq), _lib.ptr(w), 2, 0.0, -1, K, NPROBE, _lib.ptr(D),
                                     _lib.ptr(I)) == -1
    # the Python layer checks the operand's shape before the library reads it
    with pytest.raises(ValueError):
        idx.search_window(xq, K, q_pmz, 2, 0.0, 'interval')
    with pytest.raises(ValueError):
        sl._search_batch(world.q, 2, 'open', windows=w[:-1])
    # interval mode with a NULL precursor_window: every fused entry point
    null = lambda P, windows, nq: setattr(P, 'precursor_mode', 2)
    sl._interval_windows = null
    try:
        for call in (lambda: sl._search_batch(world.q, 2, 'open', windows=w),
                     lambda: sl._search_batch(world.q, 2, 'std', windows=w),
                     lambda: sl.search_batch_topn(world.q, 2, 'open', 3, windows=w)):
            with pytest.raises(_lib.AnnSoloMiError, match=ERR_INVALID) as e:
                call()
            assert 'precursor_window' in str(e.value)
    finally:
        del sl._interval_windows
    P = _params(sl, 2, None)
    qs = _lib.peaks_struct(world.q)
    knn = np.zeros((NQ, K), np.int64)
    out = np.empty(NQ, np.int32), np.empty(NQ, np.float64)
    assert L.asl_rescore_knn(sl.partitions[2].handle, C.byref(qs), C.byref(P), _lib.ptr(knn), _lib.ptr(out[0]),
                             _lib.ptr(out[1]), None, None, None, 0) == -1
    # what the window scan refuses it refuses in interval mode too, with the same messages
    def both(index, x, qk, wk, k=16):
        msgs = []
        for args in ((qk, 2, 50.0, 'Da'), (wk, 2, 0.0, 'interval')):
            with pytest.raises(_lib.AnnSoloMiError, match=ERR_STATE) as e:
                index.search_window(x, k, *args)
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], msgs
    flat = world.library('flat')[0]._get_ann_index(2)
    both(flat, xq, q_pmz, w)                          # IVF-Flat
    rng = np.random.default_rng(3)
    x = np.zeros((3000, 800), np.float32)
    for i in range(len(x)):
        x[i, rng.choice(800, 20, replace=False)] = rng.random(20)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    pq = faiss.IndexIVFPQ(faiss.IndexFlatIP(800), 800, 8, 32, 8)
    pq.set_niter(3)
    pq.train(x)
    pq.add(x)
    keyx = np.linspace(400, 1400, len(x)).astype(np.float32)
    pq.set_window_key(keyx)
    pq.nprobe = 4
    qk = keyx[:8].astype(np.float64)
    wk = np.stack([qk - 25.0, qk + 25.0], 1)
    _, I = pq.search_window(x[:8], 16, wk, 2, 0.0, 'interval')
    assert (I[:, 0] >= 0).all()
    pq.set_scan_variant(1)                            # the generic kernel
    both(pq, x[:8], qk, wk)
    pq.set_scan_variant(0)
    both(pq, x[:8], qk, wk, k=1281)                   # k above the tiled set-mode limit
    pq.shard(0, 2)                                    # a sharded index
    both(pq, x[:8], qk, wk)


def test_open_level_of_the_cascade(world):
    """Config.precursor_window_open and the queries' isolation windows reach the open level: its batches are
    the windows= batches."""
    from ann_solo_amd.spectral_library import open_window_intervals
    sl, _ = world.library('pq')
    q = world.q
    seen = []
    real = sl._search_batch

    def spy(queries, charge, mode, *a, **kw):
        seen.append((mode, kw.get('windows')))
        return real(queries, charge, mode, *a, **kw)
    qmeta = {2: [{'identifier': f'scan={i}', 'index': i, 'precursor_mz': float(world.q_pmz[i]), 'precursor_charge': 2}
                 for i in range(NQ)]}
    lmeta = {2: [{'identifier': r, 'peptide': f'PEP{r}', 'precursor_mz': float(world.key0[r])}
                 for r in range(len(world.key0))]}
    sl._search_batch = spy
    old = sl.config.precursor_window_open
    try:
        sl.config.precursor_window_open = (-50.0, 250.0)
        t = sl.search_packed({2: q}, qmeta, lmeta, score_ssms=_nothing_at_level_one)
        opened = [w for m, w in seen if m == 'open']
        assert len(opened) == 1 and [w for m, w in seen if m == 'std'] == [None]
        assert np.array_equal(opened[0], open_window_intervals(world.q_pmz, 2, (-50.0, 250.0)))
        assert np.array_equal(opened[0], world.wins['m50_p250'])
        want = real(q, 2, 'open', windows=world.wins['m50_p250'])
        got = {int(r): int(l) for r, l in zip(t.qrow, t.lib_row)}
        assert got == {i: int(want.best_row[i]) for i in range(NQ) if want.best_row[i] >= 0}
        md = t.mass_diffs()
        assert ((md >= -50.0 - 1e-3) & (md <= 250.0 + 1e-3)).all() and len(md) > 0
        # isolation windows in the metadata take the place of the derived intervals
        del seen[:]
        for i, m in enumerate(qmeta[2]):
            m['isolation_window'] = (world.q_pmz[i] - 1.0, world.q_pmz[i] + 3.0)
        sl.search_packed({2: q}, qmeta, lmeta, score_ssms=_nothing_at_level_one)
        opened = [w for m, w in seen if m == 'open']
        assert len(opened) == 1 and np.array_equal(opened[0], world.wins['iso4'])
    finally:
        sl.config.precursor_window_open = old
        del sl._search_batch


def _nothing_at_level_one(ssms, mode):
    """a scorer that accepts nothing at the standard level, so every query reaches the open level"""
    for s in ssms:
        s.search_engine_score, s.q = 0.0, (1.0 if mode == 'std' else 0.0)
    return ssms
