"""How unusual is the best match's score for THIS query: an expectation value from the score
histogram of the query's candidates (``asl_*_topn_hist``; include/annsolo_mi.h: ASL_SCORE_HIST_BINS).

The device counts the exact scores of all of a query's scored candidates into 128 bins of width 1/128
over [0, 1]. Here, on the host and vectorised over queries, the winner is taken out and a straight line
is fitted to the log of the survival counts of the losers' upper tail -- the plain log-linear tail fit
of the sequence-database engines -- and read at the winner's score: the number of candidates expected
to score at least as high by chance. It is a descriptive statistic of one query's candidate scores,
NOT a calibrated p-value: nothing says the tail is exponential, and with a few hundred candidates the
fit rests on a handful of bins. Its use is as a rescoring feature (its log) that is comparable between
a query with 160 candidates and one with 350 000, which a raw score is not. DESIGN.md 3.
"""
import numpy as np

BINS = 128          # ASL_SCORE_HIST_BINS
MIN_LOSERS = 10     # fewer losers: no value
MIN_POINTS = 3      # fewer fit points: no value


def bin_of(score) -> np.ndarray:
    """Histogram bin of an exact score ``s >= 0``, as the device computes it:
    ``127 if not s < 1.0 else int(s * 128.0)`` -- lower edges inclusive (the product is exact, so
    this is floor(128 s)), everything at or above 1 in the top bin."""
    s = np.asarray(score, np.float64)
    below = s < 1.0
    return np.where(below, np.floor(np.where(below, s, 0.0) * float(BINS)), BINS - 1).astype(np.int64)


def loser_hist(hist, best_score) -> np.ndarray:
    """The histograms ``[nq, 128]`` with one count removed from the bin of each query's best score
    ``[nq]``: the distribution of the ``N = n_cand - 1`` losers. A query without candidates (an
    all-zero row) stays as it is; a row whose winner's bin is empty is a ``ValueError``."""
    h = np.array(hist, dtype=np.int64, ndmin=2)
    s = np.atleast_1d(np.asarray(best_score, np.float64))
    if h.shape != (len(s), BINS):
        raise ValueError(f'loser_hist: histograms {h.shape} for {len(s)} best scores; [nq, {BINS}] and [nq]')
    rows = np.nonzero(h.sum(axis=1) > 0)[0]
    b = bin_of(s[rows])
    if (h[rows, b] <= 0).any():
        raise ValueError("loser_hist: a best score's bin is empty (not the histogram of that batch)")
    h[rows, b] -= 1
    return h


def expect_value(loser_hist, best_score) -> np.ndarray:
    """Expected number of candidates that score at least ``best_score`` by chance, per query ``[nq]``,
    from the losers' histograms ``[nq, 128]`` (``loser_hist``). With B = 128 and N = sum of the row:

    1. ``C[b]`` = losers in bins >= b;
    2. ``t`` = the highest non-empty loser bin;
    3. ``a`` = the lowest bin with ``C[a] <= N / 2`` (past the bulk of the distribution);
    4. ordinary least squares of ``log10 C[b]`` on ``b / B`` over ``b = a .. t``: slope m, intercept c;
    5. ``min(N, 10 ** (c + m * best_score))``.

    NaN when ``N < 10``, when there are fewer than 3 fit points, or when the slope is not negative."""
    h = np.array(loser_hist, dtype=np.int64, ndmin=2)
    s = np.atleast_1d(np.asarray(best_score, np.float64))
    if h.shape != (len(s), BINS):
        raise ValueError(f'expect_value: histograms {h.shape} for {len(s)} best scores; [nq, {BINS}] and [nq]')
    N = h.sum(axis=1)
    C = np.cumsum(h[:, ::-1], axis=1)[:, ::-1]                   # C[q, b]: losers in bins >= b
    b = np.arange(BINS)
    t = np.where(N > 0, (BINS - 1) - np.argmax(h[:, ::-1] > 0, axis=1), -1)
    past = 2 * C <= N[:, None]                                   # C[b] <= N / 2, in integers
    a = np.where(past.any(axis=1), np.argmax(past, axis=1), BINS)
    fit = (b[None, :] >= a[:, None]) & (b[None, :] <= t[:, None])    # C >= 1 on every fit point (b <= t)
    n = fit.sum(axis=1)
    x = b / float(BINS)
    y = np.log10(np.where(fit, C, 1).astype(np.float64))
    nn = np.maximum(n, 1).astype(np.float64)
    xm = (fit * x[None, :]).sum(axis=1) / nn
    ym = (fit * y).sum(axis=1) / nn
    dx = np.where(fit, x[None, :] - xm[:, None], 0.0)
    dy = np.where(fit, y - ym[:, None], 0.0)
    sxx = (dx * dx).sum(axis=1)
    ok = (N >= MIN_LOSERS) & (n >= MIN_POINTS)
    m = (dx * dy).sum(axis=1) / np.where(ok, sxx, 1.0)
    c = ym - m * xm
    ok &= m < 0.0
    with np.errstate(over='ignore'):
        e = np.minimum(N.astype(np.float64), 10.0 ** (c + m * s))
    return np.where(ok, e, np.nan)
