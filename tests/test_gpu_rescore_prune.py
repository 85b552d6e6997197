"""Pruning of deferred candidates in the rescoring (csrc/rescore.hip): a candidate with a doubly
matched peak whose upper bound -- the sum of all its generated matches -- lies below the query's
best exact score is dropped instead of going to the pair kernel, and the pair kernel walks a work
list of the queries that still have deferred candidates.

The cases of tests/prune_cases.py (tests/test_rescore_prune_cpu.py shows what they plant) through
asl_rescore_batch (the kernels' FORM 0) and, (a) - (d), asl_rescore_knn (FORM 2); a window-only
search (FORM 3); ranked requests, which never prune; pipelined batches. Every result is compared
with the oracle bit for bit -- winner, score, candidate count, match count and match list -- and the
kernels' counters (asl_profile_rescore_counts) with the CPU count of deferred and pruned candidates."""
import ctypes as C

import numpy as np
import pytest

import prune_cases as PC

pytestmark = pytest.mark.gpu


class _Counted:
    """Counters on (profiling level 1) and cleared on entry; .deferred / .pruned / .items on exit."""

    def __enter__(self):
        from ann_solo_amd import _lib
        self.L = _lib.lib()
        self.L.asl_profile_enable(1)
        self.L.asl_profile_reset()
        return self

    def __exit__(self, *exc):
        from ann_solo_amd import _lib
        d, p, w = C.c_int64(), C.c_int64(), C.c_int64()
        try:
            _lib.check(self.L.asl_profile_rescore_counts(C.byref(d), C.byref(p), C.byref(w)))
        finally:
            self.L.asl_profile_enable(0)
        self.deferred, self.pruned, self.items = d.value, p.value, w.value
        return False


def _items(n_left):
    """Work-list items of a query with n_left surviving deferred candidates (rs_pair_blocks)."""
    return min((n_left + 7) // 8, 8)


def _check_rescore_batch(O, case, want):
    from ann_solo_amd import spectrum_match
    q, lib = case.packed()
    rows, off = case.csr()
    with _Counted() as cnt:
        best, score, count, pairs = spectrum_match.rescore_batch(q, lib, rows, off, PC.TOL, True)
    Q, L = O.Spectra(*case.queries), O.Spectra(*case.library)
    for qi in range(case.nq):
        b, s, m = O.best_match(Q, qi, L, case.lists[qi], PC.TOL, True)
        assert best[qi] == b, (case.name, qi, int(best[qi]), b)
        assert score[qi] == s and count[qi] == len(m), (case.name, qi, float(score[qi]), s)
        assert pairs[qi, :len(m)].tolist() == m.tolist(), (case.name, qi)
    print('%s rescore_batch: deferred %d pruned %d items %d' % (case.name, cnt.deferred, cnt.pruned, cnt.items))
    assert cnt.deferred == sum(w[0] for w in want), case.name
    assert cnt.pruned == sum(w[1] for w in want), case.name
    assert cnt.items == sum(_items(w[0] - w[1]) for w in want), case.name
    return best


def _check_rescore_knn(O, case, want):
    """FORM 2: the packed-record path over an asl_library_t; ties go to the lowest row, so the oracle
    sees the list in ascending row. Two slots of every row stay -1."""
    import torch
    from ann_solo_amd.distributed import HipShardBackend
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    q, lib = case.packed()
    K = PC.N_CAND + 2
    cfg = Config.open_search(num_list=1 << 20, num_candidates=K, fragment_mz_tolerance=PC.TOL,
                             precursor_tolerance_mass_open=1e12, precursor_tolerance_mode_open='Da')
    sl = SpectralLibrary(lib, config=cfg)
    try:
        part = sl.partitions[2]
        assert part.spectra.n == lib.n
        knn = np.full((case.nq, K), -1, np.int64)
        for qi, rows in enumerate(case.lists):
            knn[qi, 1:1 + len(rows)] = rows
        with _Counted() as cnt:
            res = HipShardBackend(sl, 2, 'open').rescore_knn(q, torch.from_numpy(knn).to(sl.device))
        Q, P = O.Spectra(*case.queries), O.Spectra(*part.spectra.to('cpu').numpy())
        for qi in range(case.nq):
            cand = np.sort(case.lists[qi])
            b, s, m = O.best_match(Q, qi, P, cand, PC.TOL, True)
            assert res.n_candidates[qi] == len(cand), (case.name, qi)
            assert res.best_row[qi] == cand[b], (case.name, qi, int(res.best_row[qi]), int(cand[b]))
            assert res.best_score[qi] == s and res.pm_count[qi] == len(m), (case.name, qi)
            assert res.pm_pairs[qi, :len(m)].tolist() == m.tolist(), (case.name, qi)
        print('%s rescore_knn: deferred %d pruned %d items %d' % (case.name, cnt.deferred, cnt.pruned, cnt.items))
        assert cnt.deferred == sum(w[0] for w in want), case.name
        assert cnt.pruned == sum(w[1] for w in want), case.name
        assert cnt.items == sum(_items(w[0] - w[1]) for w in want), case.name
        return res
    finally:
        sl.shutdown()


@pytest.fixture(scope='module')
def counts(O):
    """The CPU count of every case, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = PC.expected_counts(O, PC.get(name))
        return cache[name]
    return get


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd'])
def test_planted_cases_both_forms(O, counts, name):
    """(a) a deferred winner with the highest bound; (b) bound above, score below the best exact
    score; (c) a tie between a deferred candidate and its plain twin, decided by position here and by
    row there; (d) every candidate deferred."""
    case, want = PC.get(name), counts(name)
    best = _check_rescore_batch(O, case, want)
    res = _check_rescore_knn(O, case, want)
    if name == 'c':
        for qi in range(case.nq):
            base = int(case.lists[qi].min())
            assert case.lists[qi][best[qi]] == base + case.notes['x_local']      # first slot: X
            assert res.best_row[qi] == base + case.notes['y_local']              # lowest row: Y
    if name == 'a':
        for qi in range(case.nq):
            assert res.best_row[qi] == int(case.lists[qi].min()) + case.notes['winner_local']


def test_list_longer_than_a_super_chunk(O, counts):
    """(e) 1 030 candidates: deferred ones in the first super-chunk, pruned only against the best
    exact score, which sits in the second."""
    case, want = PC.get('e'), counts('e')
    assert want[0][1] == want[0][0] >= 20
    best = _check_rescore_batch(O, case, want)
    assert best[0] == case.notes['winner_local']


def test_negative_intensity_is_never_pruned(O, counts):
    """(f) the sum of all matches bounds nothing when a product is negative."""
    case, want = PC.get('f'), counts('f')
    assert all(w[0] >= 8 and w[1] == 0 for w in want)
    _check_rescore_batch(O, case, want)


def test_more_deferred_candidates_than_the_list_holds(O):
    """300 deferred candidates with low bounds in one list: the kernel's list of prunable candidates
    holds 256 (RF_DLIST), the others are kept -- more work, the same result."""
    rng = np.random.default_rng(8)
    q = PC._query(rng, 37)
    cands = [PC.plain(rng, q[0], q[1], 0.60)] + [PC.twin(rng, q[0], q[1], 0.10, 0.005) for _ in range(300)]
    case = PC._assemble('overflow', [(q, cands, None)])
    (n_def, n_pruned, rec, best), = PC.expected_counts(O, case)
    assert n_def == n_pruned == 300
    want = [(300, 256, rec, best)]
    _check_rescore_batch(O, case, want)


def test_window_only_search(O, counts):
    """(g) FORM 3: a window-only search over the library of case (a); every row is in every query's
    window, the lowest row wins ties."""
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    a = PC.get('a')
    q, lib = a.packed()
    every = np.arange(lib.n, dtype=np.int64)
    case = PC.Case('g', a.queries, a.library, [every] * a.nq)
    want = PC.expected_counts(O, case)
    assert sum(w[1] for w in want) > 0
    cfg = Config.open_search(mode='bf', fragment_mz_tolerance=PC.TOL, precursor_tolerance_mass=20,
                             precursor_tolerance_mode='ppm', precursor_tolerance_mass_open=300,
                             precursor_tolerance_mode_open='Da')
    sl = SpectralLibrary(lib, config=cfg)
    try:
        part = sl.partitions[2]
        assert part.spectra.n == lib.n
        with _Counted() as cnt:
            res = sl._search_batch(q, 2, 'open')
        Q, P = O.Spectra(*a.queries), O.Spectra(*part.spectra.to('cpu').numpy())
        for qi in range(a.nq):
            b, s, m = O.best_match(Q, qi, P, every, PC.TOL, True)
            assert res.n_candidates[qi] == lib.n and res.best_row[qi] == every[b], qi
            assert res.best_score[qi] == s and res.pm_count[qi] == len(m), qi
            assert res.pm_pairs[qi, :len(m)].tolist() == m.tolist(), qi
        print('window: deferred %d pruned %d items %d' % (cnt.deferred, cnt.pruned, cnt.items))
        assert cnt.deferred == sum(w[0] for w in want)
        assert cnt.pruned == sum(w[1] for w in want)
    finally:
        sl.shutdown()


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_ranked_requests_never_prune(O, counts, name):
    """(h) n_best = 3: every deferred candidate is scored (the third best may be one), the pruned
    counter stays 0, the ranks are the oracle's best match applied three times."""
    from ann_solo_amd import spectrum_match
    from test_gpu_topn import _check_query, _oracle_ranks
    case, want = PC.get(name), counts(name)
    q, lib = case.packed()
    rows, off = case.csr()
    with _Counted() as cnt:
        top = spectrum_match.rescore_batch_topn(q, lib, rows, off, PC.TOL, True, 3)
    assert cnt.pruned == 0 and cnt.deferred == sum(w[0] for w in want)
    assert cnt.items == sum(_items(w[0]) for w in want)
    Q, L = O.Spectra(*case.queries), O.Spectra(*case.library)
    for qi in range(case.nq):
        ranks = _oracle_ranks(O, Q, qi, L, case.lists[qi], 3, PC.TOL, True)
        _check_query(top[0][qi], top[1][qi], top[2][qi], top[3][qi], [(p, s, m) for p, _, s, m in ranks], 3,
                     (name, qi))


def test_pipelined_batches_of_different_sizes():
    """(i) two batches in flight on the pipeline's streams, 512 and 200 queries: flags and work list
    live in the scratch of the stream's owner and are cleared per batch. Results and counters equal
    the synchronous calls'."""
    import torch
    from ann_solo_amd import synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, aux = synthetic.make_library(6000, seed=91, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, 512, seed=92, charge=2)
    cfg = Config.open_search(num_list=32, num_probe=8, num_candidates=128, index='ivfpq', kmeans_niter=4)
    sl = SpectralLibrary(lib, config=cfg)
    fields = ('best_row', 'best_score', 'n_candidates', 'pm_count', 'pm_pairs')
    try:
        q1 = q.to('cuda:0').contiguous()
        q2 = q.select(torch.arange(100, 300)).to('cuda:0').contiguous()
        sl._search_batch(q1, 2, 'open', device_out=True)           # (index and buffers exist)
        with _Counted() as sync_cnt:
            s1 = sl._search_batch(q1, 2, 'open', device_out=True)
            s2 = sl._search_batch(q2, 2, 'open', device_out=True)
            torch.cuda.synchronize()
        assert sync_cnt.deferred > 0 and sync_cnt.pruned > 0
        sl.set_pipeline(True)
        try:
            with _Counted() as pipe_cnt:
                p1 = sl._search_batch(q1, 2, 'open', device_out=True)
                p2 = sl._search_batch(q2, 2, 'open', device_out=True)
                p3 = sl._search_batch(q1, 2, 'open', device_out=True)
                sl.synchronize()
        finally:
            sl.set_pipeline(False)
        for got, ref in ((p1, s1), (p2, s2), (p3, s1)):
            for f in fields:
                assert torch.equal(getattr(got, f), getattr(ref, f)), f
        d1 = sync_cnt
        print('sync: deferred %d pruned %d items %d; pipelined (a third batch = the first again): %d %d %d'
              % (d1.deferred, d1.pruned, d1.items, pipe_cnt.deferred, pipe_cnt.pruned, pipe_cnt.items))
        # p3 repeats the first batch: the pipelined totals are the synchronous ones plus batch 1 again
        with _Counted() as one_cnt:
            sl._search_batch(q1, 2, 'open', device_out=True)
            torch.cuda.synchronize()
        for f in ('deferred', 'pruned', 'items'):
            assert getattr(pipe_cnt, f) == getattr(sync_cnt, f) + getattr(one_cnt, f), f
    finally:
        sl.shutdown()
