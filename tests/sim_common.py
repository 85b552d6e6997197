"""Shared helpers of the similarity-feature tests (CPU oracle and GPU kernel)."""
import os

import numpy as np

# (method, args as written in the reference test, top) -> feature column
COLUMN = {
    ('cosine', '', False): 0, ('cosine', '', True): 1, ('n_matched_peaks', '', False): 2,
    ('frac_n_peaks_query', '', False): 3, ('frac_n_peaks_library', '', False): 4,
    ('frac_n_peaks_library', '', True): 5, ('frac_intensity_query', '', False): 6,
    ('frac_intensity_library', '', False): 7, ('frac_intensity_library', '', True): 8,
    ('mean_squared_error', "'mz'", False): 9, ('mean_squared_error', "'mz'", True): 10,
    ('mean_squared_error', "'intensity'", False): 11,
    ('mean_squared_error', "'intensity'", True): 12,
    ('spectral_contrast_angle', '', False): 13, ('spectral_contrast_angle', '', True): 14,
    ('hypergeometric_score', '', False): 15, ('kendalltau', '', False): 16,
    ('ms_for_id_v1', '', False): 17, ('ms_for_id_v2', '', False): 18,
    ('entropy', 'False', False): 19, ('entropy', 'True', False): 20,
    ('entropy', 'weighted=False', False): 19, ('entropy', 'weighted=True', False): 20,
    ('entropy', '', False): 19,
    ('scribe_fragment_acc', '', False): 21, ('scribe_fragment_acc', '', True): 22,
    ('manhattan', '', False): 23, ('euclidean', '', False): 24, ('chebyshev', '', False): 25,
    ('pearsonr', '', False): 26, ('pearsonr', '', True): 27, ('spearmanr', '', False): 28,
    ('spearmanr', '', True): 29, ('braycurtis', '', False): 30, ('canberra', '', False): 31,
    ('ruzicka', '', False): 32}


# the feature row of an SSM without peak matches (column 15, the hypergeometric score, depends on
# the library's peak count)
NO_MATCH = {0: 0.0, 1: 0.0, 2: 0.0, 3: 0.0, 4: 0.0, 5: 0.0, 6: 0.0, 7: 0.0, 8: 0.0, 9: np.inf,
            10: np.inf, 11: np.inf, 12: np.inf, 13: 0.0, 14: 0.0, 16: 0.0, 17: 0.0, 18: 0.0,
            19: 0.0, 20: 0.0, 21: 0.0, 22: 0.0, 23: np.inf, 24: np.inf, 25: np.inf, 26: 0.0,
            27: 0.0, 28: 0.0, 29: 0.0, 30: 1.0, 31: np.inf, 32: 0.0}


def kat_case(kat, name):
    return (kat[f'{name}_q_mz'], kat[f'{name}_q_intensity'], kat[f'{name}_l_mz'],
            kat[f'{name}_l_intensity'], kat[f'{name}_peak_matches'].astype(np.uint32))


class EdgeCases:
    """tests/golden/ssm_features_edges.npz: one SSM per branch of the feature kernel, the
    reference's values in `features` [n, 33] and, at top = `tops`, in `features_top`
    [n, len(tops), len(top_columns)] (NaN where the reference defines none)."""

    def __init__(self):
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                                 'ssm_features_edges.npz'))
        self.g = g
        self.names = [str(s) for s in g['names']]
        self.n = len(self.names)
        self.qo, self.lo, self.po = g['q_offsets'], g['l_offsets'], g['pm_offsets']
        self.features, self.features_top = g['features'], g['features_top']
        self.tops, self.top_columns = [int(t) for t in g['tops']], g['top_columns']
        self.nq, self.nl, self.cnt = np.diff(self.qo), np.diff(self.lo), np.diff(self.po).astype(np.int32)

    def case(self, c):
        """(q_mz, q_intensity, l_mz, l_intensity, pairs [n, 2]) of case c."""
        g, q, l, p = self.g, slice(self.qo[c], self.qo[c + 1]), slice(self.lo[c], self.lo[c + 1]), \
            slice(self.po[c], self.po[c + 1])
        return g['q_mz'][q], g['q_intensity'][q], g['l_mz'][l], g['l_intensity'][l], g['pm_pairs'][p]

    def pairs(self, sel=None, stride=None):
        """Padded pair array [len(sel), stride, 2] and counts of the cases `sel`."""
        sel = range(self.n) if sel is None else sel
        cnt = self.cnt[list(sel)]
        pairs = np.zeros((len(cnt), stride or max(1, int(cnt.max())), 2), np.uint32)
        for i, c in enumerate(sel):
            pairs[i, :cnt[i]] = self.case(c)[4]
        return pairs, cnt


def check_features(got, want, tag, rel=1e-5, abs_=5e-6):
    """Feature vectors agree to `rel`/`abs_`; the contrast angle inherits arccos' sensitivity
    near cosine = 1 (d angle = (2/pi) sqrt(2 d cos))."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    for f in range(len(want)):
        a, b = got[f], want[f]
        if np.isinf(b) or np.isnan(b):
            assert (np.isnan(a) and np.isnan(b)) or a == b, (tag, f, a, b)
            continue
        tol = abs_ + rel * abs(b)
        if f in (13, 14) and want[f - 13] > 0.999:
            tol = 1e-3
        assert abs(a - b) <= tol, (tag, f, a, b)


def check_top_features(got, want_top, top_columns, tag, **kw):
    """The `*_top` columns of the feature vector `got` against `want_top` (one value per entry
    of `top_columns`); a NaN in `want_top` = the reference defines no value: 0 is expected.
    Returns the number of such entries."""
    want = np.zeros(len(got))
    want[top_columns] = np.where(np.isnan(want_top), 0.0, want_top)
    masked = np.zeros(len(got))
    masked[top_columns] = np.asarray(got, np.float64)[top_columns]
    check_features(masked, want, tag, **kw)
    return int(np.isnan(want_top).sum())
