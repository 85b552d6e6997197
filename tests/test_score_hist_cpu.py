"""The score histogram and the expectation value without a GPU: the three `asl_*_topn_hist` symbols and
their argument contract, `score_stats.bin_of` on the bin edges, `score_stats.expect_value` against a scalar
restatement of its rule, the `Config.score_stats` flag, and the cascade driver with the option on over the
oracle-backed engine (a numpy histogram over the oracle's scores)."""
import argparse
import math

import numpy as np
import pytest

from ann_solo_amd import score_stats
from ann_solo_amd.config import Config, add_arguments

B = 128


def _has_device():
    from ann_solo_amd import _lib
    return _lib.lib().asl_get_num_gpus() > 0


# ------------------------------------------------------------------ C ABI
def test_exports_and_header():
    import os
    from ann_solo_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                               'annsolo_mi.h')).read()
    for name in ('asl_rescore_batch_topn_hist', 'asl_search_batch_topn_hist', 'asl_rescore_knn_topn_hist'):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert ('int %s(' % name) in header
    assert '#define ASL_SCORE_HIST_BINS 128' in header
    assert _lib.SCORE_HIST_BINS == score_stats.BINS == B


def test_bad_rank_counts_come_first():
    """n_best outside 1 .. 16 is ASL_ERR_INVALID before anything touches the device, as for the _topn calls."""
    from ann_solo_amd import _lib
    L = _lib.lib()
    for bad in (0, 17, -1):
        assert L.asl_rescore_batch_topn_hist(None, None, None, None, None, 0.02, 1, bad, 0, None, None, None, None, 0,
                                             None) == -1
        assert b'n_best' in L.asl_last_error()
        assert L.asl_search_batch_topn_hist(None, None, None, None, bad, 0, None, None, None, None, None, 0, None,
                                            None) == -1
        assert b'n_best' in L.asl_last_error()
        assert L.asl_rescore_knn_topn_hist(None, None, None, None, bad, 1, None, None, None, None, None, 0, None) == -1
        assert b'n_best' in L.asl_last_error()


@pytest.mark.skipif(_has_device(), reason='checks the behaviour without a HIP device')
def test_compute_entry_points_need_a_device():
    from ann_solo_amd import _lib
    L = _lib.lib()
    assert L.asl_rescore_batch_topn_hist(None, None, None, None, None, 0.02, 1, 2, 0, None, None, None, None, 0,
                                         None) == -2
    assert L.asl_search_batch_topn_hist(None, None, None, None, 3, 0, None, None, None, None, None, 0, None, None) == -2
    assert L.asl_rescore_knn_topn_hist(None, None, None, None, 16, 1, None, None, None, None, None, 0, None) == -2


# ------------------------------------------------------------------ bin_of
def test_bin_of_on_the_edges():
    k = np.arange(0, B + 1)
    edge = k / float(B)
    assert np.array_equal(score_stats.bin_of(edge), np.minimum(k, B - 1))          # lower edges inclusive
    below = np.nextafter(edge[1:], 0.0)
    assert np.array_equal(score_stats.bin_of(below), k[1:] - 1)
    below32 = np.nextafter(edge[1:].astype(np.float32), np.float32(0)).astype(np.float64)
    assert np.array_equal(score_stats.bin_of(below32), k[1:] - 1)
    assert score_stats.bin_of(0.0) == 0 and score_stats.bin_of(1.0) == B - 1 and score_stats.bin_of(1.5) == B - 1
    assert score_stats.bin_of(np.nextafter(1.0, 0.0)) == B - 1
    assert score_stats.bin_of(np.array([0.45]))[0] == 57                            # floor(57.6)


# ------------------------------------------------------------------ expect_value
def _scalar_expect(h, s):
    """The rule of the issue, one query, plain Python."""
    h = [int(v) for v in h]
    N = sum(h)
    C = [sum(h[b:]) for b in range(B)]
    if N < 10:
        return float('nan')
    t = max(b for b in range(B) if h[b] > 0)
    past = [b for b in range(B) if C[b] <= N / 2]
    if not past:
        return float('nan')
    a = past[0]
    pts = [(b / B, math.log10(C[b])) for b in range(a, t + 1)]
    if len(pts) < 3:
        return float('nan')
    n = len(pts)
    xm = math.fsum(x for x, _ in pts) / n
    ym = math.fsum(y for _, y in pts) / n
    m = math.fsum((x - xm) * (y - ym) for x, y in pts) / math.fsum((x - xm) ** 2 for x, _ in pts)
    c = ym - m * xm
    if not m < 0:
        return float('nan')
    return min(float(N), 10.0 ** (c + m * s))


def _random_hists(rng, n):
    """loser histograms of every kind: geometric-ish tails, sparse ones, a heavy top bin, short tails, tiny N."""
    H = np.zeros((n, B), np.int64)
    for i in range(n):
        kind = i % 6
        size = int(rng.choice([3, 9, 10, 11, 40, 160, 5000, 350000]))
        if kind == 0:
            sc = rng.exponential(0.04, size)
        elif kind == 1:
            sc = rng.beta(2, 12, size)
        elif kind == 2:
            sc = np.concatenate([rng.exponential(0.02, size), np.full(size, 1.0)])      # more than half on top
        elif kind == 3:
            sc = np.full(size, 0.3)                                                       # one bin
        elif kind == 4:
            sc = np.concatenate([np.full(size, 0.1), np.full(size // 3, 0.11)])           # two bins
        else:
            sc = rng.uniform(0, 1.2, size)
        H[i] = np.bincount(score_stats.bin_of(sc), minlength=B)
    return H


def test_expect_value_equals_the_scalar_rule():
    rng = np.random.default_rng(3)
    H = _random_hists(rng, 240)
    s = rng.uniform(0.0, 1.0, len(H))
    got = score_stats.expect_value(H, s)
    want = np.array([_scalar_expect(H[i], s[i]) for i in range(len(H))])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = ~np.isnan(want)
    assert fin.sum() > 60 and (~fin).sum() > 60
    assert np.allclose(got[fin], want[fin], rtol=1e-12, atol=0.0)
    assert (got[fin] <= H[fin].sum(axis=1)).all() and (got[fin] > 0).all()
    assert (got[fin] < H[fin].sum(axis=1)).any() and (got[fin] == H[fin].sum(axis=1)).any()    # clipped and not
    one = score_stats.expect_value(H[5], s[5])                                       # a single query
    assert one.shape == (1,) and (one[0] == got[5] or np.isnan(got[5]))


def test_expect_value_scales_and_decreases():
    rng = np.random.default_rng(4)
    H = np.stack([np.bincount(score_stats.bin_of(rng.exponential(0.05, 20000)), minlength=B) for _ in range(8)])
    s = np.full(len(H), 0.9)
    e1, e2 = score_stats.expect_value(H, s), score_stats.expect_value(2 * H, s)
    assert np.isfinite(e1).all() and (e1 < H.sum(axis=1)).all()                      # not clipped
    assert np.allclose(e2, 2.0 * e1, rtol=1e-9)
    grid = np.linspace(0.5, 1.0, 41)
    for h in H:
        e = score_stats.expect_value(np.tile(h, (len(grid), 1)), grid)
        assert (e < h.sum()).all() and (np.diff(e) < 0).all()                        # strictly decreasing


def test_expect_value_nan_exactly_when_stated():
    def ev(h, s=0.5):
        return float(score_stats.expect_value(np.asarray(h)[None, :], [s])[0])
    base = np.zeros(B, np.int64)
    tail = base.copy()
    tail[[2, 3, 4, 5, 6]] = (6, 2, 1, 1, 1)             # N = 11; C = 11 5 3 2 1 from bin 2: a = 3, t = 6, 4 points
    assert np.isfinite(ev(tail))
    few = tail.copy()
    few[2] = 4                                           # N = 9 < 10
    assert few.sum() == 9 and math.isnan(ev(few))
    ten = tail.copy()
    ten[2] = 5                                           # N = 10: C = 10 5 3 2 1, a = 3
    assert ten.sum() == 10 and np.isfinite(ev(ten))
    two = base.copy()
    two[[2, 3, 4]] = (20, 5, 3)                          # C = 28 8 3: a = 3, t = 4 -> 2 points
    assert math.isnan(ev(two))
    three = base.copy()
    three[[2, 3, 4, 5]] = (20, 5, 3, 1)                  # a = 3, t = 5 -> 3 points
    assert np.isfinite(ev(three))
    top = base.copy()
    top[[1, 127]] = (5, 6)                               # more than half in the top bin: no bin past the bulk ...
    assert math.isnan(ev(top))
    flat = base.copy()
    flat[[0, 9]] = (12, 12)                              # C = 12 on bins 1 .. 9: slope 0, not negative
    assert math.isnan(ev(flat))
    assert math.isnan(ev(base))                          # no losers at all
    for h in (tail, few, ten, two, three, top, flat, base):
        a, b = ev(h), _scalar_expect(h, 0.5)
        assert (math.isnan(a) and math.isnan(b)) or math.isclose(a, b, rel_tol=1e-12)


def test_loser_hist_removes_the_winner():
    h = np.zeros((3, B), np.int32)
    h[0, [3, 57]] = (4, 1)
    h[2, 127] = 2
    out = score_stats.loser_hist(h, [0.45, 0.0, 1.0])
    assert out[0, 57] == 0 and out[0, 3] == 4 and out[1].sum() == 0 and out[2, 127] == 1
    assert h[0, 57] == 1                                 # the input is not written
    with pytest.raises(ValueError):
        score_stats.loser_hist(h, [0.9, 0.0, 1.0])      # bin 115 of query 0 is empty
    with pytest.raises(ValueError):
        score_stats.loser_hist(h[:, :100], [0.45, 0.0, 1.0])


# ------------------------------------------------------------------ the flag
def test_flag_parsing_validation_and_hashes():
    from ann_solo_amd.spectral_library import SpectralLibrary
    assert Config().score_stats is False
    p = argparse.ArgumentParser()
    add_arguments(p)
    assert p.parse_args([]).score_stats is False
    ns = p.parse_args(['--score_stats'])
    assert ns.score_stats is True and Config.from_reference(ns).score_stats is True
    assert Config(score_stats=True, num_gpus=1).score_stats
    with pytest.raises(ValueError, match='score_stats'):
        Config(score_stats=True, num_gpus=2)
    for index in ('ivfflat', 'ivfpq'):
        out = []
        for on in (False, True):
            sl = SpectralLibrary.__new__(SpectralLibrary)
            sl.config = Config.open_search(index=index, score_stats=on)
            out.append((sl._get_hyperparameter_hash(), sl._get_index_hash()))
        assert out[0] == out[1]


def test_ssm_record_fields_default():
    from ann_solo_amd.spectrum import SpectrumSpectrumMatch
    old = SpectrumSpectrumMatch('PEPTIDE', 'q1', 0, 7, 1.0, 2, 500.0, 499.9, False, 0.5, 0.0, np.zeros((0, 2)))
    assert old.n_scored == 0 and math.isnan(old.expect)


# ------------------------------------------------------------------ the engine, oracle-backed
def test_engine_columns_and_unchanged_identifications(O, monkeypatch):
    from ann_solo_amd import spectrum_similarity
    import score_hist_ref as R
    from oracle_backend import oracle_cosines
    monkeypatch.setattr(spectrum_similarity, 'ssm_cosine', oracle_cosines)
    lib, qs, qmeta, lmeta, kw = R.engine_case()

    seen = {}

    def gate(table, mode):                           # columnar scorer: reads both columns, accepts everything
        seen[mode] = (table.n_scored.copy(), table.expect.copy())
        table.q[:] = 0.0
    gate.columnar = True
    on = R.oracle_engine(lib, kw, score_stats=True).search_packed(qs, qmeta, lmeta, score_ssms=gate)
    seen_on = dict(seen)
    off = R.oracle_engine(lib, kw).search_packed(qs, qmeta, lmeta, score_ssms=gate)
    assert len(on) == len(off) > 30
    for name in ('charge', 'qrow', 'lib_row', 'score', 'q'):
        assert np.array_equal(getattr(on, name), getattr(off, name)), name
    for i in range(len(on)):
        assert np.array_equal(on._peak_matches(i), off._peak_matches(i))
    assert off.n_scored.shape == (len(off),) and not off.n_scored.any() and np.isnan(off.expect).all()
    assert on.n_scored.dtype == np.int32 and (on.n_scored > 0).all()
    # both kinds of value occur: level 1 scores a handful of candidates, the open level a few hundred
    fin = np.isfinite(on.expect)
    assert fin.any() and (~fin).any()
    assert (on.n_scored[fin] > 10).all() and (on.n_scored[~fin] < 11).any()
    assert (on.expect[fin] > 0).all() and (on.expect[fin] <= on.n_scored[fin] - 1).all()
    assert set(seen_on) == {'std', 'open'} and np.isfinite(seen_on['open'][1]).any()
    # recomputed from the batch-level histograms
    eng = R.oracle_engine(lib, kw, score_stats=True)
    q = qs[2]
    tops = {mode: eng.search_batch_topn(q, 2, mode, 1, score_hist=True) for mode in ('std', 'open')}
    n_std = len(seen_on['std'][0])
    for i in range(len(on)):
        top = tops['std' if i < n_std else 'open']
        r = int(on.qrow[i])
        assert on.n_scored[i] == top.n_candidates[r] == top.score_hist[r].sum()
        best = top.best_score[r, :1]
        want = score_stats.expect_value(score_stats.loser_hist(top.score_hist[r][None, :], best), best)[0]
        assert (math.isnan(want) and math.isnan(on.expect[i])) or want == on.expect[i], i
    rec = on[int(np.nonzero(fin)[0][0])]
    assert rec.n_scored > 10 and rec.expect > 0
    both = type(on).concat([on.take(fin), on.take(~fin)])
    assert len(both) == len(on) and np.isfinite(both.expect[:fin.sum()]).all() and both.n_scored.sum() == on.n_scored.sum()
