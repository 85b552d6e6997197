"""The cascade's FDR step (``utils.score_ssms``, /root/reference/src/ann_solo/utils.py:69-201) as a columnar
scorer of ``SpectralLibrary`` (``Config.device_fdr``): called as ``scorer(table, mode)`` it reads and writes
the columns of an ``SSMTable``.

  * ``CosineTDC``      -- ``--model none``: target-decoy q-values on the cosine, per precursor-mass-difference
    group at the open level (``tdc_qvalues``, ``ssm_groups``).
  * ``PercolatorTDC``  -- ``--model svm``: a Percolator-like semi-supervised linear SVM over the reference's
    feature table (``feature_table``, ``FeatureScaler``), trained on the device by ``asl_l2svm_fit`` /
    ``asl_linear_scores`` (csrc/l2svm.hip), then the same q-values on its calibrated scores.

The reference delegates the training procedure to mokapot (``PercolatorModel`` + ``brew``), which is not
vendored with it; ``PercolatorTDC`` RESTATES that procedure (DESIGN.md 3 "Rescoring model") and claims no bit
parity with mokapot.

  * ``ForestTDC``      -- ``--model rf`` WITH ``--device_forest``: the same procedure around a histogram forest
    grown and evaluated on the device by ``asl_forest_fit`` / ``asl_forest_predict`` (csrc/forest.hip). It is a
    restatement too -- a binned forest, not scikit-learn's exact-split one (DESIGN.md 3 "Rescoring model:
    forest") -- so ``--model rf`` alone does not stand for it: without the switch ``rf`` is not provided.

All three take ``qvalues='device'`` (``Config.device_qvalues``): their target-decoy q-values then come from
``asl_tdc_qvalues`` (csrc/tdc.hip) instead of ``tdc_qvalues`` / ``_grouped_q`` below, byte for byte the same; and
``groups='device'`` (``Config.device_groups``): the open level's group labels then come from ``asl_ssm_groups``
(csrc/groups.hip) instead of ``ssm_groups`` below, byte for byte the same, and the scorer keeps the modification
profile of the level as ``group_profile``."""
import logging
from typing import Optional

import numpy as np

from .spectrum_similarity import FEATURE_NAMES

__all__ = ['tdc_qvalues', 'ssm_groups', 'CosineTDC', 'feature_table', 'FeatureScaler', 'PercolatorTDC',
           'ForestTDC', 'MODEL_COLUMNS', 'make_scorer']

#: the model's columns in the key order of the reference's feature dictionary (utils.py:297-340); ``index``,
#: ``sequence`` and ``is_target`` are metadata, not features
MODEL_COLUMNS = ['sequence_len', 'precursor_charge_2', 'precursor_charge_3', 'precursor_charge_4',
                 'precursor_charge_5', 'query_prec_mz', 'lib_prec_mz', 'mz_diff_ppm', 'abs_mz_diff_ppm',
                 'mz_diff_da', 'abs_mz_diff_da'] + list(FEATURE_NAMES)
#: columns whose non-finite values become the column's finite maximum (utils.py:106-117)
_CLIPPED = ('mse_mz', 'mse_int', 'mse_mz_top5', 'mse_int_top5', 'manhattan', 'euclidean', 'chebyshev', 'canberra')
GRID = tuple((neg, pos) for neg in (0.1, 1.0, 10.0) for pos in (0.1, 1.0, 10.0))     # neg-major
INNER_FOLDS = 3
# The stop rule of every fit: ||g|| <= max(GTOL_ABS, GTOL_REL * ||g at the start||); H >= I puts the point within
# that of the minimiser. g is a sum whose addends are of the order of ||g at a zero start||, each rounded to 2^-53
# relative: 1e-13 of it is a thousand roundings of g, and ends a cold-started problem where 1e-9 lies below them.
# (At 10^6 rows the line search stalls sooner still, near ||g|| = 1e-5: DESIGN.md 3 says why that is left so.)
GTOL_ABS, GTOL_REL = 1e-9, 1e-13


def tdc_qvalues(scores, is_target, desc: bool = True) -> np.ndarray:
    """q-values by target-decoy competition (mokapot ``qvalues.tdc``): walking the matches from
    best to worst, FDR = (#decoys + 1) / #targets (1 where there is no target yet); matches of
    equal score form one step that takes the FDR at its END; q = the smallest FDR at this or
    any worse step, never above 1. Returned in input order, for targets and decoys alike."""
    scores = np.asarray(scores, np.float64)
    target = np.asarray(is_target, bool)
    if scores.shape != target.shape or scores.ndim != 1:
        raise ValueError('scores and is_target: 1-D arrays of one length')
    if np.isnan(scores).any():
        raise ValueError('scores must not hold NaN')
    n = len(scores)
    if n == 0:
        return np.zeros(0, np.float64)
    order = np.argsort(-scores if desc else scores, kind='stable')
    s, t = scores[order], target[order]
    cum_t = np.cumsum(t)
    cum_d = np.cumsum(~t)
    fdr = np.ones(n, np.float64)
    np.divide(cum_d + 1, cum_t, out=fdr, where=cum_t != 0)
    last = np.nonzero(np.append(s[1:] != s[:-1], True))[0]      # a run of equal scores ends here
    run_fdr = np.minimum(fdr[last], 1.0)
    run_q = np.minimum.accumulate(run_fdr[::-1])[::-1]          # min over this and worse runs
    run_of = np.searchsorted(last, np.arange(n), side='left')
    q = np.empty(n, np.float64)
    q[order] = run_q[run_of]
    return q


def ssm_groups(mass_diffs, min_group_size: int) -> np.ndarray:
    """Group labels from the precursor mass differences (``utils._get_ssm_groups``, :204-274):
    per nominal mass difference a 100-bin histogram over [nominal - 0.5, nominal + 0.5], its
    peaks (``scipy.signal.find_peaks`` with prominences), every SSM to the NEAREST peak (left bin
    edge) among those whose bases enclose it; groups smaller than ``min_group_size`` and
    unassigned SSMs -> -1. The reference's loop closes a run when the nominal mass changes OR at
    the very last SSM (which joins the run it closes only with the same nominal mass): an SSM that
    is last in mass order and alone in its interval is never assigned, and a single SSM never is."""
    import scipy.signal
    md = np.asarray(mass_diffs, np.float64)
    n = len(md)
    groups = -np.ones(n, np.int32)
    if n == 0:
        return groups
    order = np.argsort(md)
    nominal = np.rint(md[order])                 # round(): half to even
    starts = np.nonzero(np.append(True, nominal[1:] != nominal[:-1]))[0]
    ends = np.append(starts[1:], n)
    group = 0
    for a, b in zip(starts, ends):
        if (b == n and b - a == 1 and n > 1) or n == 1:
            continue
        members = order[a:b]
        g = nominal[a]
        bins = np.linspace(g - 0.5, g + 0.5, 101)
        hist, _ = np.histogram(md[members], bins=bins)
        peaks, prom = scipy.signal.find_peaks(hist, prominence=(None, None))
        if len(peaks):
            x = md[members][:, None]
            inside = (bins[prom['left_bases']][None, :] < x) & (x < bins[prom['right_bases']][None, :])
            dist = np.where(inside, np.abs(bins[peaks][None, :] - x), np.inf)
            best = np.argmin(dist, axis=1)       # first of equal distances, like the strict <
            ok = np.isfinite(dist[np.arange(len(members)), best])
            groups[members[ok]] = group + best[ok].astype(np.int32)
        group += len(peaks)
    labels, counts = np.unique(groups, return_counts=True)
    groups[np.isin(groups, labels[counts < min_group_size])] = -1
    return groups


def _level_groups(table, mode: str, min_group_size: int) -> np.ndarray:
    if mode == 'open':
        return ssm_groups(table.mass_diffs(), min_group_size)
    return np.zeros(len(table), np.int32)


def _grouped_q(scores, target, groups) -> np.ndarray:
    q = np.full(len(scores), np.nan)
    for g in np.unique(groups):
        m = groups == g
        q[m] = tdc_qvalues(scores[m], target[m])
    return q


def _device_tdc(device):
    """``tdc(scores, target, group=None, use=None, desc=True, fdr=None)`` over ``asl_tdc_qvalues`` (csrc/tdc.hip):
    the columns go to ``device``, ``q`` -- and the labels where ``fdr`` is given -- come back as numpy."""
    from . import _lib

    def tdc(scores, target, group=None, use=None, desc=True, fdr=None):
        import torch

        def put(a, dtype):
            if a is None or hasattr(a, 'data_ptr'):      # (a column that is on the device already stays there)
                return a
            return torch.as_tensor(np.ascontiguousarray(a, dtype)).to(device)
        out = _lib.tdc_qvalues(put(scores, np.float64), put(target, np.uint8), put(group, np.int32),
                               put(use, np.uint8), desc, fdr)
        return out.cpu().numpy() if fdr is None else tuple(o.cpu().numpy() for o in out)
    return tdc


def _as_index(rows, device):
    import torch
    return torch.as_tensor(np.ascontiguousarray(rows, np.int64)).to(device)


def _check_qvalues(qvalues):
    if qvalues not in (None, 'device'):
        raise ValueError(f"qvalues = {qvalues!r}: None (numpy on the host) or 'device' (asl_tdc_qvalues)")
    return qvalues


def _check_groups(groups):
    if groups not in (None, 'device'):
        raise ValueError(f"groups = {groups!r}: None (ssm_groups on the host) or 'device' (asl_ssm_groups)")
    return groups


class _OpenLevelGroups:
    """The group column of a level, for the three scorers (they set ``groups``, ``qvalues``, ``device``,
    ``min_group_size`` and ``fdr``). ``groups=None``: ``ssm_groups`` on the host. ``groups='device'``
    (``Config.device_groups``): the open level's labels are one ``asl_ssm_groups`` call on ``device`` (csrc/groups.hip;
    DESIGN.md 3 "Mass-difference groups"), the same bytes; with ``qvalues='device'`` the column stays a device
    tensor and goes straight into ``asl_tdc_qvalues``, and ``n_groups`` is the call's ``n_labels``. After such an
    open call ``group_profile`` holds the modification profile of the level as numpy columns: ``group`` (the ids
    that remain, ascending, then -1), ``mass`` (the left edge of the group's histogram bin; NaN for -1), ``size``
    (SSMs of the group; the rows sum to the table's length) and ``accepted`` (its targets with ``q < fdr``). Mass
    differences that span more than ``ASL_GROUPS_MAX_SPAN`` intervals: one warning, ``ssm_groups`` on the host for
    that call (the same labels) and no profile; a non-finite mass difference: ``ValueError``."""
    group_profile = None

    def _level_labels(self, table, mode: str):
        """``(group column, its number of distinct labels or None)``; numpy unless both switches are 'device'."""
        self.group_profile, self._peaks = None, None
        if mode != 'open' or self.groups is None or len(table) == 0:
            return _level_groups(table, mode, self.min_group_size), None
        import torch
        from . import _lib
        md = table.mass_diffs()
        try:
            g, n_labels, mass, size = _lib.ssm_groups(
                torch.as_tensor(np.ascontiguousarray(md, np.float64)).to(self.device), self.min_group_size, True)
        except _lib.AnnSoloMiError as e:
            if e.code == _lib.ERR_INVALID:
                raise ValueError(f'non-finite precursor mass differences at the open level: {e}') from e
            if e.code != _lib.ERR_CAPACITY:
                raise
            logging.warning('the mass differences of this open level span more than %d intervals: its groups come '
                            'from ssm_groups on the host (%s)', _lib.GROUPS_MAX_SPAN, e)
            return ssm_groups(md, self.min_group_size), None
        self._peaks = (g, mass.cpu().numpy(), size.cpu().numpy())
        return (g if self.qvalues == 'device' else g.cpu().numpy()), n_labels

    def _publish_profile(self, target, q):
        """``group_profile`` of the open call whose labels ``_level_labels`` took from the device; ``q [n]`` with
        NaN where a row has none."""
        if self._peaks is None:
            return
        g, mass, size = self._peaks
        self._peaks = None
        g = g.cpu().numpy()
        kept = np.nonzero((size > 0) & (size >= self.min_group_size))[0]
        hit = np.bincount(g[np.asarray(target, bool) & (np.asarray(q) < self.fdr)] + 1, minlength=len(size) + 1)
        self.group_profile = dict(
            group=np.append(kept, -1).astype(np.int32), mass=np.append(mass[kept], np.nan),
            size=np.append(size[kept], len(g) - size[kept].sum()).astype(np.int64),
            accepted=np.append(hit[kept + 1], hit[0]).astype(np.int64))


class CosineTDC(_OpenLevelGroups):
    """The reference's ``--model none``: q-values from the cosine by target-decoy competition, grouped by
    mass difference for the open level (utils.py:118, :139-142). Targets get their cosine as
    ``search_engine_score`` and a q-value; decoys keep NaN for both (mokapot's confidence table lists targets
    only, utils.py:186-200), so the ``q < fdr`` gate drops them. ``qvalues='device'`` (``Config.device_qvalues``):
    the grouped q-values are one ``asl_tdc_qvalues`` call on ``device`` instead of numpy -- the same bytes.
    ``groups='device'`` (``Config.device_groups``): ``_OpenLevelGroups``; ``fdr`` is the level ``group_profile``
    counts its accepted targets at."""
    columnar = True

    def __init__(self, min_group_size: int = 100, qvalues=None, device='cuda', groups=None, fdr: float = 0.01):
        self.min_group_size = int(min_group_size)
        self.groups, self.fdr = _check_groups(groups), float(fdr)
        self.n_groups: Optional[int] = None      # of the last grouped call (utils.py:127-131)
        self.qvalues, self.device = _check_qvalues(qvalues), device     # 'device': one grouped asl_tdc_qvalues call

    def __call__(self, table, mode: str):
        target = ~table.is_decoy()
        cos = np.asarray(table.score, np.float64)
        groups, n_labels = self._level_labels(table, mode)
        if mode == 'open':
            self.n_groups = len(np.unique(groups)) if n_labels is None else n_labels
        q = _grouped_q(cos, target, groups) if self.qvalues is None else \
            _device_tdc(self.device)(cos, target, group=groups)
        table.q = np.where(target, q, np.nan)
        self._publish_profile(target, table.q)
        table.score = np.where(target, cos, np.nan)
        return None


def feature_table(table):
    """The model's feature table of the SSMs of ``table`` that have peak matches (the reference skips the
    others, utils.py:344-345): ``(rows, F)`` with ``rows`` the indices into ``table`` and ``F [len(rows),
    len(MODEL_COLUMNS)]`` float64 in ``MODEL_COLUMNS`` order. ``sequence_len`` is the length of the library
    record's ``peptide``; the charge flags, precursor m/z columns and their differences are formed as
    ``spectrum_similarity.compute_ssm_features`` forms them; the 33 similarity columns are ``table.features``
    (the batches' ``ssm_features``); non-finite values of the eight distance columns become the column's
    finite maximum."""
    if len(table) == 0:         # a level that filed no batch: nothing to score, whatever columns it carries
        return np.zeros(0, np.int64), np.zeros((0, len(MODEL_COLUMNS)))
    feats = np.asarray(getattr(table, 'features', np.zeros((len(table), 0))), np.float64)
    if feats.shape != (len(table), len(FEATURE_NAMES)):
        raise ValueError(f'the table carries no similarity features ({feats.shape}): the level must run with '
                         'ssm_features (SpectralLibrary does with a PercolatorTDC scorer)')
    n_matched = feats[:, FEATURE_NAMES.index('n_matched_peaks')]
    rows = np.nonzero(np.isfinite(n_matched) & (n_matched > 0))[0]
    sub = table.take(rows)
    pep = sub._column(sub.library_meta, sub.lib_row, 'peptide', object)
    z = sub._column(sub.query_meta, sub.qrow, 'precursor_charge', np.int64)
    q_pmz = sub._column(sub.query_meta, sub.qrow, 'precursor_mz', np.float64)
    l_pmz = sub._column(sub.library_meta, sub.lib_row, 'precursor_mz', np.float64)
    ppm = (q_pmz - l_pmz) / l_pmz * 10 ** 6
    head = [np.fromiter((len(p) for p in pep), np.float64, len(rows)),
            z <= 2, z == 3, z == 4, z >= 5, q_pmz, l_pmz, ppm, np.abs(ppm), q_pmz - l_pmz, np.abs(q_pmz - l_pmz)]
    F = np.concatenate([np.stack([np.asarray(c, np.float64) for c in head], axis=1), feats[rows]], axis=1)
    for name in _CLIPPED:
        col = F[:, MODEL_COLUMNS.index(name)]
        fin = np.isfinite(col)
        if not fin.all() and fin.any():
            col[~fin] = col[fin].max()
    return rows, F


class FeatureScaler:
    """``make_pipeline(StandardScaler(), VarianceThreshold(), CorrelationThreshold(0.95))`` of the reference
    (utils.py:23-66, :147-151), fitted in float64: centre and scale by the population standard deviation (a
    constant column keeps scale 1, as sklearn's), drop the columns without variance, then every column whose
    absolute correlation with an EARLIER kept column exceeds the threshold."""

    def __init__(self, threshold: float = 0.95):
        self.threshold = float(threshold)

    def fit(self, X) -> 'FeatureScaler':
        """``X [n, d]``: numpy, or a torch tensor -- the statistics are then computed where it lives (on the
        device for the device solver: they are plumbing, and the matrix is there anyway)."""
        if hasattr(X, 'data_ptr'):
            return self._fit_torch(X)
        X = np.asarray(X, np.float64)
        n = X.shape[0]
        self.mean_ = X.mean(axis=0)
        var = X.var(axis=0)
        self.scale_ = np.where(self._constant(var, self.mean_, n), 1.0, np.sqrt(var))
        Z = (X - self.mean_) / self.scale_
        keep = np.minimum(Z.var(axis=0), np.ptp(Z, axis=0)) > 0        # VarianceThreshold(0)
        kept = np.nonzero(keep)[0]
        corr = np.abs(np.corrcoef(Z[:, kept], rowvar=False)) if len(kept) > 1 else np.zeros((1, 1))
        return self._select(keep, kept, corr)

    def _fit_torch(self, X) -> 'FeatureScaler':
        import torch
        X = X.to(torch.float64)
        mean, var = X.mean(dim=0), X.var(dim=0, unbiased=False)
        self.mean_, var = mean.cpu().numpy(), var.cpu().numpy()
        self.scale_ = np.where(self._constant(var, self.mean_, X.shape[0]), 1.0, np.sqrt(var))
        Z = (X - mean) / torch.as_tensor(self.scale_, device=X.device)
        spread = torch.minimum(Z.var(dim=0, unbiased=False), Z.amax(dim=0) - Z.amin(dim=0))
        keep = (spread > 0).cpu().numpy()
        kept = np.nonzero(keep)[0]
        corr = np.zeros((1, 1))
        if len(kept) > 1:
            corr = torch.corrcoef(Z[:, torch.as_tensor(kept, device=X.device)].T).abs().cpu().numpy()
        return self._select(keep, kept, corr)

    @staticmethod
    def _constant(var, mean, n):
        eps = np.finfo(np.float64).eps      # sklearn's constant-feature test (_is_constant_feature)
        return var <= n * eps * var + (n * mean * eps) ** 2

    def _select(self, keep, kept, corr) -> 'FeatureScaler':
        if len(kept) > 1:                   # CorrelationThreshold.fit (utils.py:61-62)
            keep[kept[(np.tril(corr, k=-1) > self.threshold).any(axis=1)]] = False
        self.support_ = keep
        return self

    def transform(self, X):
        """The kept columns of ``(X - mean) / scale``, C-contiguous; numpy or torch as ``X`` is."""
        if hasattr(X, 'data_ptr'):
            import torch
            mean, scale = (torch.as_tensor(v, device=X.device) for v in (self.mean_, self.scale_))
            cols = torch.as_tensor(np.nonzero(self.support_)[0], device=X.device)
            return ((X.to(torch.float64) - mean) / scale)[:, cols].contiguous()
        X = np.asarray(X, np.float64)
        return np.ascontiguousarray(((X - self.mean_) / self.scale_)[:, self.support_])

    def fit_transform(self, X):
        return self.fit(X).transform(X)


class _Fallback(Exception):
    pass


def _device_solver(device):
    """(fit, scores) over ``asl_l2svm_fit`` / ``asl_linear_scores`` with the matrix resident on ``device``."""
    from . import _lib

    def prepare(X):
        import torch
        return torch.as_tensor(X, dtype=torch.float64).to(device).contiguous()

    def scores(X, wb):
        out = _lib.linear_scores(X, wb)
        return out.cpu().numpy() if hasattr(out, 'cpu') else out
    return _lib.l2svm_fit, scores, prepare


class _SemiSupervisedTDC(_OpenLevelGroups):
    """The procedure ``PercolatorTDC`` and ``ForestTDC`` share (mokapot's ``brew``, restated; the steps are listed
    under ``PercolatorTDC``): folds, start labels from the cosine, the parameter choice once per fold, ``max_iter``
    relabelling rounds, calibration, grouped TDC, the fallbacks and the ``trace``. A model supplies four hooks:

      ``_open()``                      -> ``(ctx, prepare)``: the solver and where it wants the matrix;
      ``_model_input(ctx, X, train)``  -> what the solver reads in place of the scaled matrix (default: ``X``);
      ``_choose(ctx, X, lab, held)``   -> ``(grid point, mean held-out accuracies)``;
      ``_round(ctx, X, lab, best, tr, state)`` -> ``(scores of all rows, state)``: one fit on the labelled rows.

    ``qvalues``: ``None`` -- every target-decoy competition is ``tdc_qvalues`` in numpy; ``'device'``
    (``Config.device_qvalues``) -- each is one ``asl_tdc_qvalues`` call on ``device`` (csrc/tdc.hip; DESIGN.md 3
    "Target-decoy q-values"): the labels of a round with the training rows as ``use``, the held-out q, the grouped
    q with ``group``. The bytes are the same; ``trace['labels']`` stays numpy. ``groups``: ``_OpenLevelGroups``."""
    columnar = True
    uses_features = True        # SpectralLibrary: the level keeps the batches' 33 similarity columns

    def __init__(self, fdr: float = 0.01, min_group_size: int = 100, folds: int = 3, max_iter: int = 10,
                 seed: int = 1, solver=None, device='cuda', qvalues=None, groups=None):
        if folds < 2 or max_iter < 1:
            raise ValueError(f'{type(self).__name__}: folds >= 2 and max_iter >= 1')
        self.fdr, self.min_group_size = float(fdr), int(min_group_size)
        self.folds, self.max_iter, self.seed = int(folds), int(max_iter), int(seed)
        self.solver, self.device = solver, device
        # None: numpy on the host; 'device': every TDC of the procedure is one asl_tdc_qvalues call (the same bytes)
        self._tdc = _device_tdc(device) if _check_qvalues(qvalues) == 'device' else None
        self.qvalues, self.groups = qvalues, _check_groups(groups)
        self.fallback = False
        self.n_groups: Optional[int] = None
        self.trace: list = []
        self.n_fit_calls = 0

    def _model_input(self, ctx, X, train):
        return X

    def _labels(self, scores, target, train, desc=True):
        """(+1 target with q <= fdr, 0 other target, -1 decoy) over the rows ``train``, 0 elsewhere."""
        if self._tdc is not None:
            use = np.zeros(len(scores), np.uint8)
            use[train] = 1
            return self._tdc(scores, target, use=use, desc=desc, fdr=self.fdr)[1]
        lab = np.zeros(len(scores), np.int8)
        q = tdc_qvalues(scores[train], target[train], desc)
        t = target[train]
        lab[train[t & (q <= self.fdr)]] = 1
        lab[train[~t]] = -1
        return lab

    def _train(self, ctx, X, target, cos, train, fold: int):
        start = [self._labels(cos, target, train, desc) for desc in (True, False)]
        lab = start[0] if (start[0] == 1).sum() >= (start[1] == 1).sum() else start[1]
        if not (lab == 1).any() or not (lab == -1).any():
            raise _Fallback('no target passes the training FDR on the cosine' if (lab == -1).any()
                            else 'a training set without decoys')
        # the parameters: grid points x 3 inner folds over the labelled rows
        labelled = np.nonzero(lab != 0)[0]
        perm = np.random.default_rng([self.seed, fold]).permutation(len(labelled))
        held = [labelled[p] for p in np.array_split(perm, INNER_FOLDS)]
        best, accuracy = self._choose(ctx, X, lab, held)
        tr = dict(grid=best, accuracy=accuracy, labels=[])
        state = None
        for it in range(self.max_iter):
            tr['labels'].append(lab.copy())
            s, state = self._round(ctx, X, lab, best, tr, state)
            if it + 1 < self.max_iter:          # (the last round's model is the model: no labels after it)
                lab = self._labels(s, target, train)
                if not (lab == 1).any():
                    raise _Fallback('no target passes the training FDR on the model score')
        self.trace.append(tr)
        return s

    def score_features(self, F, is_target, cosine, groups=None):
        """Steps 1-4 over a feature matrix ``F [m, d]``: ``(calibrated score [m], q [m])``; raises
        ``_Fallback`` where the procedure cannot run."""
        F = np.asarray(F, np.float64)
        target = np.asarray(is_target, bool)
        cos = np.asarray(cosine, np.float64)
        m = len(F)
        self.trace = []
        ctx, prepare = self._open()
        if m < self.folds or target.all() or not target.any():
            raise _Fallback('too few SSMs, or one class only')
        if not np.isfinite(F).all():        # (the reference's LinearSVC refuses them too)
            raise _Fallback('non-finite feature values')
        parts = np.array_split(np.random.default_rng(self.seed).permutation(m), self.folds)
        score = np.full(m, np.nan)
        Fs = prepare(F)                      # where the solver reads it: scaled there, once per fold
        for fold, test in enumerate(parts):
            train = np.sort(np.concatenate([p for i, p in enumerate(parts) if i != fold]))
            X = FeatureScaler().fit(Fs[train]).transform(Fs)
            if X.shape[1] == 0:
                raise _Fallback('no feature with variance')
            s = self._train(ctx, self._model_input(ctx, X, train), target, cos, train, fold)[test]
            t = target[test]
            q = tdc_qvalues(s, t) if self._tdc is None else self._tdc(s, t)
            passing = t & (q <= self.fdr)
            if not passing.any() or t.all():
                raise _Fallback('no target of a held-out part passes the FDR')
            s_t, s_d = s[passing].min(), np.median(s[~t])
            if not s_t > s_d:
                raise _Fallback('a held-out part whose targets do not score above its decoys')
            score[test] = (s - s_t) / (s_t - s_d)
        if groups is None:
            groups = np.zeros(m, np.int32)
        elif not hasattr(groups, 'data_ptr'):       # (a device column of groups='device' stays where it is)
            groups = np.asarray(groups)
        return score, (_grouped_q(score, target, groups) if self._tdc is None else
                       self._tdc(score, target, group=groups))

    # -- the scorer ---------------------------------------------------------------------------------------
    def __call__(self, table, mode: str):
        self.fallback = False
        n = len(table)
        if n == 0:              # an empty level (every query identified before it, say): nothing to score
            return None
        target = ~table.is_decoy()
        groups, n_labels = self._level_labels(table, mode)
        try:
            rows, F = feature_table(table)
            sub = groups[rows] if not hasattr(groups, 'data_ptr') else \
                groups[_as_index(rows, groups.device)].contiguous()
            score, q = self.score_features(F, target[rows], F[:, MODEL_COLUMNS.index('cosine')], sub)
        except _Fallback as e:
            logging.warning('%s falls back to the cosine (CosineTDC) for this %s level: %s', type(self).__name__,
                            mode, e)
            self.fallback = True
            gate = CosineTDC(self.min_group_size, self.qvalues, self.device, self.groups, self.fdr)
            gate(table, mode)
            self.n_groups, self.group_profile = gate.n_groups, gate.group_profile
            return None
        if mode == 'open':
            self.n_groups = len(np.unique(groups)) if n_labels is None else n_labels
        full_s, full_q = np.full(n, np.nan), np.full(n, np.nan)
        t = target[rows]
        full_s[rows[t]], full_q[rows[t]] = score[t], q[t]
        table.score, table.q = full_s, full_q
        self._publish_profile(target, full_q)
        return None


class PercolatorTDC(_SemiSupervisedTDC):
    """The reference's ``--model svm`` (mokapot's ``PercolatorModel`` under ``brew``), restated:

    1. the SSMs with peak matches are split into ``folds`` parts by a seeded permutation;
    2. per part, a model is trained on the other parts: the features are scaled (``FeatureScaler``, fitted on
       the training rows); the start labels come from the cosine by TDC at ``fdr`` in the direction that passes
       more targets (+1 target with q <= fdr, 0 other target, -1 decoy); the class weights are chosen once from
       ``GRID`` by a seeded 3-fold inner cross-validation (accuracy on the held-out labelled rows, the first of
       equal means) -- 27 problems in ONE ``l2svm_fit`` call; then ``max_iter`` rounds of fit on the rows
       labelled +-1, score the training rows, relabel by TDC at ``fdr``. The LAST round's weights are the model;
    3. every part is scored by its model and calibrated: (s - s_t) / (s_t - s_d), s_t the lowest score of a
       target passing ``fdr``, s_d the median decoy score;
    4. merged; q-values by TDC, per mass-difference group at ``mode == 'open'`` as ``CosineTDC``;
    5. targets get the calibrated score and q, decoys and SSMs without peak matches NaN for both.

    A stage without a passing target, or a training set with one class only: ``CosineTDC`` for that call, a
    warning, ``self.fallback = True``. ``solver``: the ``(fit, scores)`` pair, default the device's
    (``_lib.l2svm_fit``, ``_lib.linear_scores`` with the matrix on ``device``). ``self.trace`` keeps, per fold,
    the grid point chosen, the labels of every round and the weights, for the tests."""
    def __init__(self, fdr: float = 0.01, min_group_size: int = 100, folds: int = 3, max_iter: int = 10,
                 seed: int = 1, solver=None, device='cuda', C: float = 1.0, qvalues=None, groups=None):
        super().__init__(fdr, min_group_size, folds, max_iter, seed, solver, device, qvalues, groups)
        self.C = float(C)
        self.n_newton = 0

    def _open(self):
        if self.solver is None:
            fit, scores_of, prepare = _device_solver(self.device)
        else:
            (fit, scores_of), prepare = self.solver, (lambda X: X)
        return (fit, scores_of), prepare

    def _fit(self, fit, X, label, cw, wb=None):
        wb, _, steps, status = fit(X, label, cw, C=self.C, gtol_abs=GTOL_ABS, gtol_rel=GTOL_REL, wb=wb)
        self.n_fit_calls += 1
        self.n_newton += int(np.max(steps)) if len(steps) else 0
        if np.any(status != 0):
            logging.debug('l2svm_fit: status %s after %s Newton steps', status.tolist(), steps.tolist())
        return wb

    def _choose(self, ctx, X, lab, held):
        # class weights: 9 grid points x 3 inner folds over the labelled rows, one fit, one scoring call
        fit, scores_of = ctx
        P = len(GRID) * INNER_FOLDS
        labels = np.repeat(lab[None, :], P, axis=0)
        cw = np.zeros((P, 2))
        for g, pair in enumerate(GRID):
            for f in range(INNER_FOLDS):
                labels[g * INNER_FOLDS + f, held[f]] = 0
                cw[g * INNER_FOLDS + f] = pair
        s = scores_of(X, self._fit(fit, X, labels, cw))
        acc = np.zeros((len(GRID), INNER_FOLDS))
        for g in range(len(GRID)):
            for f in range(INNER_FOLDS):
                pred = np.where(s[g * INNER_FOLDS + f, held[f]] > 0, 1, -1)
                acc[g, f] = np.mean(pred == lab[held[f]]) if len(held[f]) else 0.0
        return int(np.argmax(acc.mean(axis=1))), acc.mean(axis=1)     # the first of equal means

    def _round(self, ctx, X, lab, best, tr, wb):
        fit, scores_of = ctx
        wb = self._fit(fit, X, lab[None, :], np.asarray([GRID[best]]), wb)
        tr.setdefault('wb', []).append(wb[0].copy())
        return scores_of(X, wb)[0], wb


#: the reference's forest grid (utils.py:156-179) in ``ParameterGrid``'s key order: class weight major, depth
#: fastest; class weights as (weight of decoys, weight of targets), ``None`` = (1, 1); depth ``None`` = 12
FOREST_CLASS_WEIGHTS = ((1.0, 1.0), (0.1, 1.0), (0.1, 10.0), (1.0, 0.1), (1.0, 10.0), (10.0, 0.1), (10.0, 1.0))
FOREST_DEPTHS = (3, 5, 7, 9, 12)
FOREST_GRID = tuple((cw, depth) for cw in FOREST_CLASS_WEIGHTS for depth in FOREST_DEPTHS)


def _forest_device_solver(device):
    """(bin, fit, predict) over ``asl_forest_*`` with the matrix and the models resident on ``device``."""
    from . import _lib

    def prepare(X):
        import torch
        return torch.as_tensor(X, dtype=torch.float64).to(device).contiguous()

    def predict(bins, d, model, max_depth=None):
        return _lib.forest_predict(bins, d, model, max_depth).cpu().numpy()
    return (_lib.forest_bin, _lib.forest_fit, predict), prepare


def forest_bin_edges(X, train):
    """``(edges [d, 255], n_edges [d])`` of the binning (DESIGN.md 3 "Rescoring model: forest"): per column of
    ``X`` the sorted values over the rows ``train`` at the ranks ``floor(k * n_train / 256)``, k = 1 .. 255,
    duplicates removed. No interpolation: the host's sort and the device's give the same edges bit for bit."""
    ranks = (np.arange(1, 256) * len(train)) // 256
    if hasattr(X, 'data_ptr'):
        import torch
        S = torch.sort(X[torch.as_tensor(train, device=X.device)], dim=0).values
        S = S[torch.as_tensor(ranks, device=X.device)].cpu().numpy() if len(train) else np.zeros((0, X.shape[1]))
    else:
        S = np.sort(np.asarray(X, np.float64)[train], axis=0)[ranks] if len(train) else np.zeros((0, X.shape[1]))
    d = int(X.shape[1])
    edges, n_edges = np.zeros((d, 255)), np.zeros(d, np.int32)
    for j in range(d if len(S) else 0):
        e = np.unique(S[:, j])
        edges[j, :len(e)], n_edges[j] = e, len(e)
    return edges, n_edges


class ForestTDC(_SemiSupervisedTDC):
    """The reference's ``--model rf`` (its default: a ``GridSearchCV(RandomForestClassifier)`` under mokapot's
    ``brew``), restated with a HISTOGRAM forest grown on the device (``Config.device_forest``; csrc/forest.hip;
    DESIGN.md 3 "Rescoring model: forest" lists every deviation from scikit-learn's exact-split forest). The five
    steps, the fallbacks and the ``trace`` are ``PercolatorTDC``'s; what differs:

    * the scaled matrix is binned per fold (``forest_bin_edges`` over the fold's training rows, ``forest_bin``);
    * the score is ``proba``, the forest's mean leaf value (mokapot: ``predict_proba[:, 1]``);
    * the grid is ``FOREST_GRID``, 7 class weights x 5 depths: the 7 x 3 problems are ONE ``forest_fit`` call at
      depth 12, the five depths five ``forest_predict`` calls on it -- a tree cut at depth d is the tree grown to
      depth d; a held-out row is predicted +1 iff ``proba > 0.5``; the first of equal mean accuracies wins;
    * every relabelling round is one ``forest_fit`` with P = 1 at the chosen depth, then one ``forest_predict``.

    ``solver``: the ``(bin, fit, predict)`` triple, default the device's (``_lib.forest_bin`` / ``forest_fit`` /
    ``forest_predict`` with the matrix on ``device``)."""

    def __init__(self, fdr: float = 0.01, min_group_size: int = 100, folds: int = 3, max_iter: int = 10,
                 seed: int = 1, solver=None, device='cuda', trees: int = 100, qvalues=None, groups=None):
        super().__init__(fdr, min_group_size, folds, max_iter, seed, solver, device, qvalues, groups)
        self.trees = int(trees)
        if self.trees < 1:
            raise ValueError('ForestTDC: trees >= 1')

    def _open(self):
        if self.solver is None:
            return _forest_device_solver(self.device)
        return tuple(self.solver), (lambda X: X)

    def _model_input(self, ctx, X, train):
        edges, n_edges = forest_bin_edges(X, train)
        return ctx[0](X, edges, n_edges), int(X.shape[1]), n_edges + 1

    def _choose(self, ctx, X, lab, held):
        (_, fit, predict), (bins, d, n_bins) = ctx, X
        P = len(FOREST_CLASS_WEIGHTS) * INNER_FOLDS
        labels = np.repeat(lab[None, :], P, axis=0)
        cw = np.zeros((P, 2))
        for g, pair in enumerate(FOREST_CLASS_WEIGHTS):
            for f in range(INNER_FOLDS):
                labels[g * INNER_FOLDS + f, held[f]] = 0
                cw[g * INNER_FOLDS + f] = pair
        model = fit(bins, d, labels, cw, trees=self.trees, max_depth=max(FOREST_DEPTHS), seed=self.seed,
                    n_bins=n_bins)
        self.n_fit_calls += 1
        acc = np.zeros((len(FOREST_CLASS_WEIGHTS), len(FOREST_DEPTHS), INNER_FOLDS))
        for k, depth in enumerate(FOREST_DEPTHS):
            proba = predict(bins, d, model, depth)
            for g in range(len(FOREST_CLASS_WEIGHTS)):
                for f in range(INNER_FOLDS):
                    pred = np.where(proba[g * INNER_FOLDS + f, held[f]] > 0.5, 1, -1)
                    acc[g, k, f] = np.mean(pred == lab[held[f]]) if len(held[f]) else 0.0
        mean = acc.mean(axis=2).reshape(-1)             # class-weight major, depth fastest: FOREST_GRID's order
        return int(np.argmax(mean)), mean               # the first of equal means

    def _round(self, ctx, X, lab, best, tr, state):
        (_, fit, predict), (bins, d, n_bins) = ctx, X
        cw, depth = FOREST_GRID[best]
        model = fit(bins, d, lab[None, :], np.asarray([cw]), trees=self.trees, max_depth=depth, seed=self.seed,
                    n_bins=n_bins)
        self.n_fit_calls += 1
        return predict(bins, d, model, depth)[0], None


def make_scorer(config, device='cuda'):
    """The scorer ``Config.device_fdr`` stands for: ``model`` None / 'none' -> ``CosineTDC``, 'svm' ->
    ``PercolatorTDC``; 'rf' with ``device_forest`` -> ``ForestTDC``; anything else (the reference's 'rf' without
    that switch included) is a ``ValueError``. ``Config.device_qvalues`` hands every scorer ``qvalues='device'``,
    ``Config.device_groups`` ``groups='device'``."""
    model = config.model
    qvalues = 'device' if getattr(config, 'device_qvalues', False) else None
    groups = 'device' if getattr(config, 'device_groups', False) else None
    if model is None or model == 'none':
        return CosineTDC(config.fdr_min_group_size, qvalues=qvalues, device=device, groups=groups, fdr=config.fdr)
    if model == 'svm':
        return PercolatorTDC(config.fdr, config.fdr_min_group_size, device=device, qvalues=qvalues, groups=groups)
    if model == 'rf' and getattr(config, 'device_forest', False):
        return ForestTDC(config.fdr, config.fdr_min_group_size, device=device, trees=config.forest_trees,
                         qvalues=qvalues, groups=groups)
    raise ValueError(f"device_fdr: model = {model!r} is not provided; None / 'none' (cosine) or 'svm'")
