"""Window-only searches (cascade level 'std', --mode bf) rescored in tiles of a bounded number of
(query, library row) pairs (asl_set_window_pair_budget):
  * on a small library with invalid rows and exact duplicates (score ties across tile
    boundaries), every budget gives the same winners, bit-equal scores, candidate counts and peak
    matches, equal to the oracle's best match over the precursor window;
  * a brute-force open search at the bench's scale (2.1 M spectra, +-500 Da, 16 384 queries) whose
    pairs pass 2^31 returns, with per-query counts equal to a host count over the float32 precursor
    column and sampled winners equal to the oracle's (ASL_BF_FULLSCALE_N overrides the size)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_FULL = int(os.environ.get('ASL_BF_FULLSCALE_N', 2_100_000))
UNLIMITED = 1 << 62


def _set_budget(pairs):
    from ann_solo_amd import _lib
    prev = _lib.lib().asl_set_window_pair_budget(pairs)
    assert prev > 0, 'asl_set_window_pair_budget rejected %d' % pairs
    return prev


def _search(sl, q, mode, budget):
    prev = _set_budget(budget)
    try:
        return sl._search_batch(q, 2, mode)
    finally:
        _set_budget(prev)


def _concat(packs):
    from ann_solo_amd.packed import PackedSpectra
    parts = [p.numpy() for p in packs]
    counts = np.concatenate([np.diff(p[0]) for p in parts])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return PackedSpectra.from_numpy(off, *(np.concatenate([p[i] for p in parts]) for i in range(1, 6)))


def _long_query(lib, rows, pmz):
    """One query of more than 100 peaks: the peaks of several library spectra, ascending m/z."""
    from ann_solo_amd.packed import PackedSpectra
    off, mz, it, ch, _, _ = lib.numpy()
    sel = np.concatenate([np.arange(off[r], off[r + 1]) for r in rows])
    mz_, order = np.unique(mz[sel], return_index=True)
    assert 100 < len(mz_) <= 256
    return PackedSpectra.from_numpy([0, len(mz_)], mz_, it[sel][order], ch[sel][order], [pmz], [2])


@pytest.fixture(scope='module')
def small():
    from ann_solo_amd import synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    base, aux = synthetic.make_library(3000, seed=7, device='cpu', charges=(2,), charge_p=(1.0,))
    rng = np.random.default_rng(11)
    dup = rng.choice(3000, 400, replace=False)
    lib = base.select(torch.as_tensor(np.concatenate([np.arange(3000), dup])))   # rows 3000.. copy rows dup
    valid = rng.random(lib.n) > 0.1
    valid[dup[:20]] = False          # an invalid original: its copy, a higher row, can win
    valid[3000:3000 + 40] = True
    valid[dup[20:40]] = True         # both valid: the tie goes to the original, the lower row
    cfg = Config.open_search(mode='bf', precursor_tolerance_mass=20, precursor_tolerance_mode='ppm',
                             precursor_tolerance_mass_open=300, precursor_tolerance_mode_open='Da')
    sl = SpectralLibrary(lib, config=cfg, valid=valid)
    ordinary, _ = synthetic.make_queries(base, aux, 48, seed=5, charge=2)
    ties = base.select(torch.as_tensor(dup[:40]))           # a library spectrum as query: exact ties
    far = ordinary.select(torch.arange(1))
    far.precursor_mz = torch.tensor([1.0e5], dtype=torch.float64)    # an empty window
    pm = base.precursor_mz.numpy()
    longq = [_long_query(base, dup[40 + 5 * i:45 + 5 * i], pm[dup[40 + 5 * i]]) for i in range(3)]
    q = _concat([ordinary, ties, far] + longq)
    special = np.array([0, 48, 48 + 20, 88, 89, 90])       # ordinary, both kinds of tie, empty, long
    yield sl, lib, valid, q, special, dup
    sl.shutdown()


def _same(a, b, rows=None):
    pick = (lambda x: x) if rows is None else (lambda x: x[rows])
    assert np.array_equal(pick(a.best_row), b.best_row)
    assert np.array_equal(pick(a.best_score).view(np.int64), b.best_score.view(np.int64))
    assert np.array_equal(pick(a.n_candidates), b.n_candidates)
    assert np.array_equal(pick(a.pm_count), b.pm_count)
    assert np.array_equal(pick(a.pm_pairs), b.pm_pairs)


@pytest.mark.parametrize('mode,tol,tmode', [('open', 300, 'Da'), ('std', 20, 'ppm')])
def test_tiles_equal_one_pass_and_the_oracle(O, small, mode, tol, tmode):
    sl, lib, valid, q, special, dup = small
    full = _search(sl, q, mode, UNLIMITED)
    total = int(full.n_candidates.astype(np.int64).sum())
    assert total > 1000 if mode == 'open' else total > 0
    for budget in (7, 1000):
        _same(_search(sl, q, mode, budget), full)
    _same(full, _search(sl, q.select(torch.as_tensor(special)), mode, 1), special)
    # the oracle over the window (valid rows whose float32 precursor passes, ascending row)
    part = sl.partitions[2]
    L = O.Spectra(*part.spectra.to('cpu').numpy())
    Q = O.Spectra(*q.numpy())
    pmz32 = part.precursor_mz
    for i in range(q.n):
        near = np.nonzero(np.abs(pmz32.astype(np.float64) - Q.precursor_mz[i]) <= 200.0)[0]
        want = np.array([r for r in near if valid[r] and
                         O.precursor_ok(Q.precursor_mz[i], pmz32[r], 2, tol, tmode)], np.int64)
        assert full.n_candidates[i] == len(want)
        b, s, m = O.best_match(Q, i, L, want, 0.02, True)
        if b < 0:
            assert full.best_row[i] == -1 and full.pm_count[i] == 0
            continue
        assert full.best_row[i] == want[b] and full.best_score[i] == s
        assert np.array_equal(full.peak_matches(i), m)
    assert full.n_candidates[88] == 0 and full.best_row[88] == -1     # the empty window
    # a library spectrum as query mostly finds itself: its copy when the original is invalid, the
    # original (the lower of two rows with the same score) when both are valid
    assert (full.best_row[48:68] == 3000 + np.arange(20)).mean() > 0.8
    assert (full.best_row[68:88] == dup[20:40]).mean() > 0.8


def _window_counts(pmz32, q_pmz, charge, tol):
    """Per query, the float32 precursors l with |q - l| * charge <= tol (Da), by np.searchsorted
    over the sorted column; the boundaries are then moved onto the exact predicate."""
    s = np.sort(pmz32.astype(np.float64))
    n = len(s)
    ok = lambda l: np.abs(q_pmz - l) * charge <= tol
    lo = np.searchsorted(s, q_pmz - tol / charge, 'left')
    hi = np.searchsorted(s, q_pmz + tol / charge, 'right')
    for _ in range(8):
        a = (lo > 0) & ok(s[np.maximum(lo - 1, 0)])                  # the row below passes too
        b = ~a & (lo < hi) & ~ok(s[np.minimum(lo, n - 1)])          # the first row fails
        c = (hi < n) & ok(s[np.minimum(hi, n - 1)])
        d = ~c & (hi > lo) & ~ok(s[np.maximum(hi - 1, 0)])
        if not (a | b | c | d).any():
            return lo, hi
        lo, hi = lo - a + b, hi + c - d
    raise AssertionError('window boundaries did not settle')


def test_bf_open_search_beyond_2_31_pairs(O):
    from ann_solo_amd import synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    dev = torch.device('cuda', 0)
    lib, aux = synthetic.make_library(N_FULL, seed=20240807, device=dev, charges=(2,), charge_p=(1.0,))
    cfg = Config.open_search(mode='bf', precursor_tolerance_mass_open=500, precursor_tolerance_mode_open='Da',
                             batch_size=16384)
    sl = SpectralLibrary(lib, config=cfg, device=dev)
    try:
        q, _ = synthetic.make_queries(lib, aux, 16384, seed=42, open_range=500.0, charge=2)
        res = sl._search_batch(q, 2, 'open')
        n = res.n_candidates.astype(np.int64)
        if N_FULL >= 2_000_000:
            assert n.sum() > 2 ** 31 - 1                # the old path's limit
        part = sl.partitions[2]
        pmz32 = part.precursor_mz
        q_pmz = q.precursor_mz.cpu().numpy()
        lo, hi = _window_counts(pmz32, q_pmz, 2, 500.0)
        assert np.array_equal(n, hi - lo)
        # sampled winners against the oracle, the widest window among them
        order = np.argsort(pmz32, kind='stable')
        rng = np.random.default_rng(3)
        sample = np.unique(np.concatenate([[int(np.argmax(n))], rng.choice(q.n, 7, replace=False)]))
        L = O.Spectra(*part.spectra.to('cpu').numpy())
        Q = O.Spectra(*q.numpy())
        for i in sample:
            want = np.sort(order[lo[i]:hi[i]]).astype(np.int64)
            b, s, m = O.best_match(Q, int(i), L, want, 0.02, True)
            assert b >= 0
            assert res.best_row[i] == want[b] and res.best_score[i] == s
            assert np.array_equal(res.peak_matches(i), m)
    finally:
        sl.shutdown()
