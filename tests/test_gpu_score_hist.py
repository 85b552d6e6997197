"""The score histogram of a query's candidates (asl_rescore_batch_topn_hist / asl_search_batch_topn_hist /
asl_rescore_knn_topn_hist, `Config.score_stats`) through the kernels. The reference histogram is
`np.bincount` of `score_stats.bin_of` over the oracle's exact score of every candidate the oracle keeps;
every comparison is exact. Beside it: the rows sum to n_cand, the histogram does not depend on n_best or
distinct, every other output equals the plain `_topn` / `_topn_distinct` call bit for bit, and a NULL
histogram is that call."""
import ctypes as C

import numpy as np
import pytest
import torch

import rescore_cases as RC
import score_hist_ref as R
from test_gpu_bf_stream import UNLIMITED, _set_budget
from test_gpu_window_scan import _window_mask

pytestmark = pytest.mark.gpu

B = 128
FIELDS = ('best_row', 'best_score', 'n_candidates', 'pm_count', 'pm_pairs')


def _bytes_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _rescore_hist(q, lib, cand, off, tol, flags, n, distinct=0, group=None, stride=8, hist='host', device=False):
    """asl_rescore_batch_topn_hist; outputs pre-filled with 0xff bytes. hist: 'host', 'device' or None (NULL).
    Returns (best_cand, best_score, pm_count, pm_pairs, hist or None) as numpy."""
    from ann_solo_amd import _lib
    nq = q.n
    outs = [np.full((nq, n), -1, np.int32), np.full((nq, n), np.nan), np.full((nq, n), -1, np.int32),
            np.full((nq, n, stride, 2), 0xffffffff, np.uint32)]
    h = None
    if hist == 'host':
        h = np.full((nq, B), -1, np.int32)
    elif hist == 'device':
        h = torch.full((nq, B), -1, dtype=torch.int32, device='cuda:0')
    if device:
        q, lib = q.to('cuda:0').contiguous(), lib.to('cuda:0').contiguous()
    _lib.check(_lib.lib().asl_rescore_batch_topn_hist(
        C.byref(_lib.peaks_struct(q)), C.byref(_lib.peaks_struct(lib)), _lib.ptr(np.ascontiguousarray(cand, np.int64)),
        _lib.ptr(np.ascontiguousarray(off, np.int32)), _lib.ptr(group), float(tol), int(flags), n, int(distinct),
        *[_lib.ptr(o) for o in outs], stride, _lib.ptr(h)))
    if hist == 'device':
        torch.cuda.synchronize()
        h = h.cpu().numpy()
    return (*outs, h)


# ------------------------------------------------------------------ 1. the bin edges
def _edge_spectra():
    """One query peak of intensity 1.0 against single-peak library spectra whose intensity IS the score."""
    from ann_solo_amd.packed import PackedSpectra
    k = np.arange(0, B + 1)
    on = (k / float(B)).astype(np.float32)
    below = np.nextafter(on[1:], np.float32(0))
    inten = np.concatenate([on, below, np.float32([1.5, 1.0])]).astype(np.float32)
    mz = np.full(len(inten), 500.0, np.float32)
    mz[-1] = 700.0                                                 # another m/z: no match, score 0
    n = len(inten)
    lib = PackedSpectra.from_numpy(np.arange(n + 1, dtype=np.int32), mz, inten, np.zeros(n, np.uint8),
                                   np.full(n, 600.0), np.full(n, 2, np.int32))
    nq = 6
    q = PackedSpectra.from_numpy(np.arange(nq + 1, dtype=np.int32), np.full(nq, 500.0, np.float32),
                                 np.ones(nq, np.float32), np.zeros(nq, np.uint8), np.full(nq, 600.0),
                                 np.full(nq, 2, np.int32))
    want = np.concatenate([on, below, np.float32([1.5, 0.0])]).astype(np.float64)
    return q, lib, want


def _edge_lists(n_lib):
    """lists of 0, 1, 63, 64, 65 and 200 slots; every fifth slot is -1, one row is listed twice; together
    they name every library row."""
    lists = []
    for n, start in ((0, 0), (1, 64), (63, 100), (64, 212), (65, 160), (200, 0)):
        c = np.full(n, -1, np.int64)
        if n == 1:
            c[0] = start
        elif n:
            slot = np.setdiff1d(np.arange(n), np.arange(2, n, 5))
            c[slot] = (start + np.arange(len(slot))) % n_lib
            c[7] = c[0]                                            # a row listed twice (in a -1 slot)
        lists.append(c)
    return lists


def test_bin_edges_on_caller_lists_and_knn_rows(O):
    from ann_solo_amd import _lib
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    from ann_solo_amd.spectrum import HASH_SEED, get_dim
    q, lib, want = _edge_spectra()
    Q, L = O.Spectra(*q.numpy()), O.Spectra(*lib.numpy())
    scores = R.pair_scores(O, Q, 0, L, np.arange(lib.n))
    assert np.array_equal(scores, want)                            # the oracle's scores are the planted values
    lists = _edge_lists(lib.n)
    assert [len(c) for c in lists] == [0, 1, 63, 64, 65, 200]
    seen = np.unique(np.concatenate(lists))
    assert np.array_equal(seen, np.arange(-1, lib.n))
    ref = np.stack([R.hist_of(scores[c[c >= 0]]) for c in lists])
    n_valid = np.array([(c >= 0).sum() for c in lists])
    assert n_valid.tolist() == [0, 1, 51, 52, 53, 161]
    every = ref.sum(axis=0)
    assert (every >= 2).all() and every[B - 1] >= 3                          # every bin; 1 and 1.5 on top
    assert ref[5, 0] == 3 and not ref[0].any() and ref[1, 64] == 1           # row 0 twice in the 200-slot list
    cand = np.concatenate(lists)
    off = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int32)
    plain = None
    for n in (1, 5):
        host = _rescore_hist(q, lib, cand, off, 0.02, 1, n, hist='host')
        dev = _rescore_hist(q, lib, cand, off, 0.02, 1, n, hist='device', device=True)
        null = _rescore_hist(q, lib, cand, off, 0.02, 1, n, hist=None)
        for got in (host[4], dev[4]):
            assert np.array_equal(got, ref), n
            assert np.array_equal(got.sum(axis=1), n_valid)
        from ann_solo_amd import spectrum_match
        plain = spectrum_match.rescore_batch_topn(q, lib, cand, off, 0.02, True, n, pm_stride=8)
        for a, b, c, d in zip(plain, host, dev, null):
            assert _bytes_equal(a, b) and _bytes_equal(a, c) and _bytes_equal(a, d), n
    # distinct ranks (caller's group column): the same histogram; without the column an error
    group = (np.arange(lib.n) // 4).astype(np.int32)
    dist = _rescore_hist(q, lib, cand, off, 0.02, 1, 5, distinct=1, group=group)
    assert np.array_equal(dist[4], ref)
    for a, b in zip(spectrum_match.rescore_batch_topn(q, lib, cand, off, 0.02, True, 5, pm_stride=8, groups=group), dist):
        assert _bytes_equal(a, b)
    assert not _bytes_equal(dist[0], plain[0])                     # (the plain ranks repeat groups)
    assert _bytes_equal(_rescore_hist(q, lib, cand, off, 0.02, 1, 5, distinct=0, group=group)[0], plain[0])
    assert _lib.lib().asl_rescore_batch_topn_hist(
        C.byref(_lib.peaks_struct(q)), C.byref(_lib.peaks_struct(lib)), _lib.ptr(cand), _lib.ptr(off), None, 0.02, 1, 5, 1,
        None, None, None, None, 0, None) == -3
    # the same lists as fixed-stride neighbour rows of a library handle: n_cand comes back too
    cfg = Config.open_search(mode='bf', precursor_tolerance_mass_open=1e12, precursor_tolerance_mode_open='Da')
    sl = SpectralLibrary(lib, config=cfg)
    try:
        K = 200
        knn = np.full((q.n, K), -1, np.int64)
        for i, c in enumerate(lists):
            knn[i, :len(c)] = c
        _, min_bound, _ = get_dim(cfg.min_mz, cfg.max_mz, cfg.bin_size)
        P = _lib.AslSearchParams(min_bound, cfg.bin_size, HASH_SEED, K, 1, 2, 1e12, 0, 0.02, 1, 0)
        qd = q.to('cuda:0').contiguous()
        for n in (1, 5):
            row, sc = np.empty((q.n, n), np.int32), np.empty((q.n, n))
            nc, cnt = np.empty(q.n, np.int32), np.empty((q.n, n), np.int32)
            hist = np.full((q.n, B), -1, np.int32)
            _lib.check(_lib.lib().asl_rescore_knn_topn_hist(
                sl.partitions[2].handle, C.byref(_lib.peaks_struct(qd)), C.byref(P), _lib.ptr(knn), n, 0,
                _lib.ptr(row), _lib.ptr(sc), _lib.ptr(nc), _lib.ptr(cnt), None, 0, _lib.ptr(hist)))
            assert np.array_equal(hist, ref) and np.array_equal(hist.sum(axis=1), nc) and np.array_equal(nc, n_valid)
            row2, sc2 = np.empty((q.n, n), np.int32), np.empty((q.n, n))
            nc2, cnt2 = np.empty(q.n, np.int32), np.empty((q.n, n), np.int32)
            _lib.check(_lib.lib().asl_rescore_knn_topn(
                sl.partitions[2].handle, C.byref(_lib.peaks_struct(qd)), C.byref(P), _lib.ptr(knn), n,
                _lib.ptr(row2), _lib.ptr(sc2), _lib.ptr(nc2), _lib.ptr(cnt2), None, 0))
            for a, b in ((row, row2), (sc, sc2), (nc, nc2), (cnt, cnt2)):
                assert _bytes_equal(a, b), n
        # distinct without a group column: an error, never the plain ranks
        assert _lib.lib().asl_rescore_knn_topn_hist(
            sl.partitions[2].handle, C.byref(_lib.peaks_struct(qd)), C.byref(P), _lib.ptr(knn), 2, 1,
            None, None, None, None, None, 0, None) == -3
        assert _lib.lib().asl_rescore_knn_topn_hist(
            None, C.byref(_lib.peaks_struct(qd)), C.byref(P), _lib.ptr(knn), 2, 0,
            None, None, None, None, None, 0, None) == -1
    finally:
        sl.shutdown()


# ------------------------------------------------------------------ 2. one bin, a list split over blocks
def test_one_bin_split_list(O):
    q, lib, want = _edge_spectra()
    one = q.select(torch.arange(1))
    n = 5000                                                       # > 4096 slots of one query: ysplit > 1
    cand = np.full(n, 37, np.int64)                                # score 37/128
    off = np.array([0, n], np.int32)
    for hist in ('host', 'device'):
        got = _rescore_hist(one, lib, cand, off, 0.02, 1, 1, hist=hist)
        assert got[4][0, 37] == n and got[4].sum() == n
        assert got[0][0, 0] == 0 and got[1][0, 0] == 37 / 128.0   # the first slot wins the tie
    cand[1::3] = -1
    cand[2::3] = 129 + 37                                          # the float32 below 38/128: bin 37 too
    got = _rescore_hist(one, lib, cand, off, 0.02, 1, 1)
    assert got[4][0, 37] == (cand >= 0).sum() and got[4].sum() == (cand >= 0).sum()
    assert got[0][0, 0] == 2


# ------------------------------------------------------------------ 3. deferred candidates
def _assert_deferred(run):
    from test_gpu_rescore_prune import _Counted
    with _Counted() as c:
        out = run()
    assert c.deferred > 0 and c.pruned == 0                        # a request with a histogram never prunes
    return out


def test_deferred_candidates_da(O):
    """The planted doubly matched peaks of tests/rescore_cases.py: the flat kernel leaves those candidates to
    the pair kernel, whose scores are counted like any other."""
    b = RC.regime_blocks(1)[0]
    assert b.tol == 0.02
    q, lib = b.packed()
    rows, off = RC.grouped_lists(b)
    Q, L = O.Spectra(*b.queries), O.Spectra(*b.library)
    ref = np.stack([R.hist_of(R.pair_scores(O, Q, i, L, rows[off[i]:off[i + 1]], b.tol, True)) for i in range(b.nq)])
    for n in (1, 3):
        got = _assert_deferred(lambda: _rescore_hist(q, lib, rows, off, b.tol, 1, n, stride=128))
        assert np.array_equal(got[4], ref), n
        assert np.array_equal(got[4].sum(axis=1), np.diff(off))
    assert (ref[:, 1:] > 0).any()


def test_deferred_candidates_ppm():
    """... and with ASL_SCORE_FRAGMENT_PPM, on the ppm-planted blocks of tests/ppm_cases.py (built from the
    same generator), against the per-peak-tolerance restatement tests/ppm_ref.py."""
    import ppm_cases as PC
    from test_gpu_ppm import _ref
    b = PC.blocks()[1]
    q, lib = b.packed()
    rows, off = PC.grouped_lists(b)
    ref = np.stack([R.hist_of([_ref(b.name, b.queries, i, b.library, int(r), b.ppm)[0] for r in rows[off[i]:off[i + 1]]])
                    for i in range(b.nq)])
    got = _assert_deferred(lambda: _rescore_hist(q, lib, rows, off, b.ppm, 3, 3, stride=128))
    assert np.array_equal(got[4], ref)
    assert np.array_equal(got[4].sum(axis=1), np.diff(off)) and (ref[:, 1:] > 0).any()


# ------------------------------------------------------------------ 4. the fused paths
class _World:
    """A 3 000-row synthetic library, 32 queries, and the oracle's score of every (query, row) pair a test asks
    for -- computed once, shared, never changed."""

    def __init__(self, O):
        from ann_solo_amd import synthetic
        self.O = O
        self.lib, aux = synthetic.make_library(3000, seed=21, device='cpu', charges=(2,), charge_p=(1.0,))
        self.q, _ = synthetic.make_queries(self.lib, aux, 32, seed=22, charge=2, open_range=300.0)
        self.q16 = self.q.select(torch.arange(16))
        self.Q, self.L = O.Spectra(*self.q.numpy()), O.Spectra(*self.lib.numpy())
        self.key = self.lib.precursor_mz.numpy().astype(np.float32)
        self.q_pmz = self.q.numpy()[4].astype(np.float64)
        self.valid = np.random.default_rng(23).random(self.lib.n) > 0.05
        self.groups = (np.arange(self.lib.n) % 40).astype(np.int32)
        self._score = {}
        self.engines = {}

    def scores(self, i, rows):
        out = np.empty(len(rows))
        for k, r in enumerate(np.asarray(rows, np.int64).tolist()):
            if (i, r) not in self._score:
                self._score[i, r] = R.pair_scores(self.O, self.Q, i, self.L, [r])[0]
            out[k] = self._score[i, r]
        return out

    def engine(self, name):
        from ann_solo_amd.spectral_library import Config, SpectralLibrary
        if name not in self.engines:
            kw = dict(precursor_tolerance_mass=20.0, precursor_tolerance_mode='ppm',
                      precursor_tolerance_mass_open=300.0, precursor_tolerance_mode_open='Da')
            if name == 'bf':
                kw.update(mode='bf')
            else:
                index, window = name.split('-')
                kw.update(num_list=16, num_probe=6, num_candidates=128, index=index, kmeans_niter=4, ann_window=window)
            sl = self.engines[name] = SpectralLibrary(self.lib, config=Config.open_search(**kw), valid=self.valid)
            sl.set_match_groups({2: self.groups})
        return self.engines[name]

    def window(self, i, mode):
        tol, tmode = (300.0, 'Da') if mode == 'open' else (20.0, 'ppm')
        return _window_mask(self.q_pmz[i], self.key, 2, tol, tmode) & self.valid

    def ref(self, cands):
        return np.stack([R.hist_of(self.scores(i, c)) for i, c in enumerate(cands)])

    def close(self):
        for sl in self.engines.values():
            sl.shutdown()


@pytest.fixture(scope='module')
def world(O):
    w = _World(O)
    yield w
    w.close()


def _hist_calls(sl, q, mode, want, what, **kw):
    """n_best 1 and 5, plain and distinct ranks: the same histogram (`want`: the oracle's, or None), the other
    outputs those of the plain calls. Returns the n_best = 5 result."""
    first = None
    for n, distinct in ((1, False), (5, False), (5, True)):
        top = sl.search_batch_topn(q, 2, mode, n, distinct=distinct, score_hist=True, **kw)
        plain = sl.search_batch_topn(q, 2, mode, n, distinct=distinct, **kw)
        for f in FIELDS:
            assert _bytes_equal(getattr(top, f), getattr(plain, f)), (what, n, distinct, f)
        if plain.knn is not None:
            assert _bytes_equal(top.knn, plain.knn), (what, n, distinct)
        assert top.score_hist.dtype == np.int32 and top.score_hist.shape == (q.n, B)
        assert np.array_equal(top.score_hist.sum(axis=1), top.n_candidates), (what, n, distinct)
        if want is not None:
            assert np.array_equal(top.score_hist, want), (what, n, distinct)
        if first is None:
            first = top
        assert _bytes_equal(top.score_hist, first.score_hist), (what, n, distinct)
    return top


def _postfilter(on):
    from ann_solo_amd import _lib
    return _lib.lib().asl_set_scan_postfilter(int(on))


@pytest.mark.parametrize('name', ['ivfpq-post', 'ivfflat-post', 'ivfpq-pre'])
def test_ann_paths(world, name):
    sl = world.engine(name)
    q = world.q
    prev = _postfilter(1)
    try:
        for post in (1, 0):
            _postfilter(post)
            knn = sl.search_batch_topn(q, 2, 'open', 1, want_knn=True).knn
            cands = []
            for i in range(q.n):
                ids = np.unique(knn[i][knn[i] >= 0])
                cands.append(ids[world.window(i, 'open')[ids]])
            want = world.ref(cands)
            assert want.sum() > 10 * q.n
            top = _hist_calls(sl, q, 'open', want, (name, post))                   # the scans' set-mode rows
            _hist_calls(sl, q, 'open', want, (name, post, 'knn'), want_knn=True)   # the ordered neighbour list
            dev = sl.search_batch_topn(q.to('cuda:0'), 2, 'open', 5, distinct=True, device_out=True, score_hist=True)
            torch.cuda.synchronize()
            assert _bytes_equal(dev.score_hist.cpu().numpy(), top.score_hist)
    finally:
        _postfilter(prev)


def _raw_params(sl, mode, use_ann, flags=1):
    from ann_solo_amd import _lib
    from ann_solo_amd.spectrum import HASH_SEED, get_dim
    cfg = sl.config
    _, min_bound, _ = get_dim(cfg.min_mz, cfg.max_mz, cfg.bin_size)
    tol, tmode = sl._tolerance(mode)
    return _lib.AslSearchParams(min_bound, cfg.bin_size, HASH_SEED, sl._num_candidates, sl._num_probe, 2, float(tol),
                                0 if tmode == 'Da' else 1, cfg.fragment_mz_tolerance, flags, int(use_ann))


def _raw_search_hist(sl, q, P, n, distinct, hist, idx=None, stride=64):
    from ann_solo_amd import _lib
    qd = q.to('cuda:0').contiguous()
    outs = [np.full((q.n, n), -1, np.int32), np.full((q.n, n), np.nan), np.full(q.n, -1, np.int32),
            np.full((q.n, n), -1, np.int32), np.full((q.n, n, stride, 2), 0xffffffff, np.uint32)]
    _lib.check(_lib.lib().asl_search_batch_topn_hist(
        sl.partitions[2].handle, idx._h if idx is not None else None, C.byref(_lib.peaks_struct(qd)), C.byref(P), n,
        int(distinct), *[_lib.ptr(o) for o in outs], stride, None, _lib.ptr(hist)))
    return outs


def test_null_histogram_is_the_plain_call(world):
    """score_hist == NULL: asl_search_batch_topn / _topn_distinct, every output, ANN and window-only; and the
    knn form equals the fused call when it is given the ids the index returned."""
    from ann_solo_amd import _lib
    for name, mode in (('ivfpq-post', 'open'), ('bf', 'open'), ('bf', 'std')):
        sl = world.engine(name)
        use_ann = name != 'bf'
        idx = sl._get_ann_index(2) if use_ann else None
        P = _raw_params(sl, mode, use_ann)
        for n, distinct in ((1, 0), (5, 0), (5, 1)):
            got = _raw_search_hist(sl, world.q16, P, n, distinct, None, idx)
            want = sl.search_batch_topn(world.q16, 2, mode, n, distinct=bool(distinct), pm_stride=64)
            for a, f in zip(got, FIELDS):
                assert _bytes_equal(a, getattr(want, f)), (name, mode, n, distinct, f)
    sl = world.engine('ivfpq-post')
    top = sl.search_batch_topn(world.q16, 2, 'open', 5, want_knn=True, score_hist=True, pm_stride=64)
    P = _raw_params(sl, 'open', True)
    qd = world.q16.to('cuda:0').contiguous()
    nq = world.q16.n
    outs = [np.empty((nq, 5), np.int32), np.empty((nq, 5)), np.empty(nq, np.int32), np.empty((nq, 5), np.int32),
            np.empty((nq, 5, 64, 2), np.uint32)]
    hist = torch.full((nq, B), -1, dtype=torch.int32, device='cuda:0')
    _lib.check(_lib.lib().asl_rescore_knn_topn_hist(
        sl.partitions[2].handle, C.byref(_lib.peaks_struct(qd)), C.byref(P), _lib.ptr(np.ascontiguousarray(top.knn)), 5, 0,
        *[_lib.ptr(o) for o in outs], 64, _lib.ptr(hist)))
    torch.cuda.synchronize()
    for a, f in zip(outs, FIELDS):
        assert _bytes_equal(a, getattr(top, f)), f
    assert _bytes_equal(hist.cpu().numpy(), top.score_hist)


@pytest.mark.parametrize('mode', ['std', 'open'])
def test_window_only_any_budget(world, mode):
    sl = world.engine('bf')
    q = world.q16
    cands = [np.nonzero(world.window(i, mode))[0] for i in range(q.n)]
    want = world.ref(cands)
    sizes = np.array([len(c) for c in cands])
    prev = _set_budget(UNLIMITED)
    try:
        full = _hist_calls(sl, q, mode, want, (mode, 'one pass'))
        assert np.array_equal(full.n_candidates, sizes)
        if mode == 'open':
            assert np.sort(sizes)[1] > 400
            # budgets below a single window: all windows but one are cut across tiles (the rows a window names,
            # invalid ones included, are what the budget counts)
            for budget in (257, 1000):
                _set_budget(budget)
                tiled = _hist_calls(sl, q, mode, want, (mode, budget))
                for f in FIELDS:
                    assert _bytes_equal(getattr(tiled, f), getattr(full, f)), (budget, f)
        else:
            assert (sizes == 0).any() or sizes.min() < 10
            _set_budget(3)
            _hist_calls(sl, q, mode, want, (mode, 3))
    finally:
        _set_budget(prev)


def test_selection_and_intervals(world):
    keep = np.random.default_rng(29).random(world.lib.n) > 0.4
    q = world.q16
    lo = world.q_pmz[:q.n] - 40.0 - np.arange(q.n)                 # asymmetric intervals of library m/z
    wins = np.stack([lo, world.q_pmz[:q.n] + 90.0], axis=1)
    inside = [(world.key.astype(np.float64) >= wins[i, 0]) & (world.key.astype(np.float64) <= wins[i, 1]) & world.valid
              for i in range(q.n)]
    prev = _set_budget(UNLIMITED)
    try:
        for name in ('bf', 'ivfpq-post'):
            sl = world.engine(name)
            sl.set_search_subset({2: keep})
            try:
                if name == 'bf':
                    cands = [np.nonzero(world.window(i, 'open') & keep)[0] for i in range(q.n)]
                else:
                    knn = sl.search_batch_topn(q, 2, 'open', 1, want_knn=True).knn
                    assert keep[knn[knn >= 0]].all()
                    cands = [np.unique(knn[i][knn[i] >= 0]) for i in range(q.n)]
                    cands = [c[world.window(i, 'open')[c]] for i, c in enumerate(cands)]
                _hist_calls(sl, q, 'open', world.ref(cands), (name, 'selection'))
                if name == 'bf':
                    _set_budget(300)
                    _hist_calls(sl, q, 'open', world.ref(cands), (name, 'selection', 300))
                    _set_budget(UNLIMITED)
            finally:
                sl.set_search_subset(None)
            if name == 'bf':
                cands = [np.nonzero(m)[0] for m in inside]
            else:
                knn = sl.search_batch_topn(q, 2, 'open', 1, want_knn=True, windows=wins).knn
                cands = [np.unique(knn[i][knn[i] >= 0]) for i in range(q.n)]
                cands = [c[inside[i][c]] for i, c in enumerate(cands)]
            assert sum(len(c) for c in cands) > 5 * q.n
            _hist_calls(sl, q, 'open', world.ref(cands), (name, 'interval'), windows=wins)
    finally:
        _set_budget(prev)


# ------------------------------------------------------------------ 5. the engine
def test_engine_score_stats(O):
    """`Config(score_stats=True)` on the case tests/test_score_hist_cpu.py runs through the oracle backend (both
    a finite value and a NaN occur there): the same table as the oracle-backed engine's, expect recomputed
    from the batch histograms, winners those of a run without the flag."""
    from ann_solo_amd import score_stats
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, qs, qmeta, lmeta, kw = R.engine_case()
    tables, engines = {}, {}
    try:
        for on in (False, True):
            sl = engines[on] = SpectralLibrary(lib, config=Config.open_search(score_stats=on, **kw))
            tables[on] = sl.search_packed(qs, qmeta, lmeta)
        t0, t1 = tables[False], tables[True]
        assert len(t0) == len(t1) > 30
        for name in ('charge', 'qrow', 'lib_row', 'score', 'q'):
            assert _bytes_equal(getattr(t0, name), getattr(t1, name)), name
        for i in range(len(t0)):
            assert np.array_equal(t0._peak_matches(i), t1._peak_matches(i)), i
        assert not t0.n_scored.any() and np.isnan(t0.expect).all()
        fin = np.isfinite(t1.expect)
        assert fin.any() and (~fin).any() and (t1.n_scored[~fin] < 11).any() and (t1.n_scored > 0).all()
        sl = engines[True]
        q = qs[2]
        tops = {mode: sl.search_batch_topn(q, 2, mode, 1, score_hist=True) for mode in ('std', 'open')}
        n_std = int((tops['std'].best_row[:, 0] >= 0).sum())    # no scorer: level 1 keeps every query it matched
        for i in range(len(t1)):
            top = tops['std' if i < n_std else 'open']
            r = int(t1.qrow[i])
            assert top.best_row[r, 0] == t1.lib_row[i] and t1.n_scored[i] == top.n_candidates[r], i
            best = top.best_score[r, :1]
            want = score_stats.expect_value(score_stats.loser_hist(top.score_hist[r][None, :], best), best)[0]
            assert (np.isnan(want) and np.isnan(t1.expect[i])) or want == t1.expect[i], i
        # the oracle-backed engine scores the same candidates: the same columns
        ref = R.oracle_engine(lib, kw, score_stats=True)
        import ann_solo_amd.spectrum_similarity as sim
        from oracle_backend import oracle_cosines
        real = sim.ssm_cosine
        sim.ssm_cosine = oracle_cosines
        try:
            tr = ref.search_packed(qs, qmeta, lmeta)
        finally:
            sim.ssm_cosine = real
        assert np.array_equal(tr.lib_row, t1.lib_row) and np.array_equal(tr.n_scored, t1.n_scored)
        assert _bytes_equal(tr.expect, t1.expect)
        rec = t1[int(np.nonzero(fin)[0][0])]
        assert rec.n_scored == t1.n_scored[np.nonzero(fin)[0][0]] and rec.expect > 0
    finally:
        for sl in engines.values():
            sl.shutdown()
