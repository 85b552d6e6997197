"""(Shifted) dot-product rescoring -- host-side mirror of the reference's
``ann_solo/spectrum_match.pyx`` (``get_best_match`` :28-108) on top of the HIP
kernels behind ``asl_rescore_batch``; ``get_best_matches`` / ``rescore_batch_topn`` report the
n best candidates instead of the single best (``asl_rescore_batch_topn``), with ``groups`` the n
best of distinct groups (``asl_rescore_batch_topn_distinct``).
"""
import numpy as np

from . import _lib
from .packed import PackedSpectra

SCORE_SHIFT, SCORE_FRAGMENT_PPM = 1, 2      # include/annsolo_mi.h: ASL_SCORE_*


def score_flags(allow_shift, fragment_tolerance_unit='Da'):
    """The C ABI's score flag word (its ``allow_shift`` argument / member): the shifted dot product
    and the unit of ``fragment_mz_tolerance`` -- ``'Da'``, or ``'ppm'`` of the query peak's m/z."""
    if fragment_tolerance_unit not in ('Da', 'ppm'):
        raise ValueError(f"fragment_tolerance_unit = {fragment_tolerance_unit!r}: 'Da' or 'ppm'")
    return (SCORE_SHIFT if allow_shift else 0) | (SCORE_FRAGMENT_PPM if fragment_tolerance_unit == 'ppm' else 0)


def get_best_match(query, candidates, fragment_mz_tolerance, allow_shift, fragment_tolerance_unit='Da'):
    """Drop-in for ``spectrum_match.get_best_match``: returns
    ``(best candidate object, score, [(query_peak, candidate_peak), ...])``.
    ``fragment_tolerance_unit='ppm'``: the tolerance is in ppm of the query peak's m/z."""
    if len(candidates) == 0:
        raise ValueError('get_best_match needs at least one candidate '
                         '(the reference guards this at spectral_library.py:359)')
    q = PackedSpectra.from_spectra([query])
    lib = PackedSpectra.from_spectra(candidates)
    offsets = np.array([0, len(candidates)], np.int32)
    rows = np.arange(len(candidates), dtype=np.int64)
    best, score, counts, pairs = rescore_batch(q, lib, rows, offsets, fragment_mz_tolerance,
                                               allow_shift, fragment_tolerance_unit=fragment_tolerance_unit)
    n = int(counts[0])
    return (candidates[int(best[0])], float(score[0]),
            [(int(a), int(b)) for a, b in pairs[0, :n]])


def get_best_matches(query, candidates, fragment_mz_tolerance, allow_shift, n, groups=None,
                     fragment_tolerance_unit='Da'):
    """The ``n`` best candidates of ``get_best_match``'s ranking, best first: a list of up to ``n``
    ``(candidate object, score, [(query_peak, candidate_peak), ...])`` (fewer when there are fewer
    candidates). Equal scores go to the earlier candidate; entry 0 is ``get_best_match``'s answer.
    ``groups``: one integer per candidate (e.g. an id of its peptide) -- the list then names up to
    ``n`` DISTINCT groups, each by its best candidate (a candidate is skipped when an earlier entry
    has its group); a negative id is "ungrouped" and never collides. ``fragment_tolerance_unit``: as in
    ``get_best_match``."""
    if len(candidates) == 0:
        raise ValueError('get_best_matches needs at least one candidate '
                         '(the reference guards this at spectral_library.py:359)')
    if groups is not None and len(groups) != len(candidates):
        raise ValueError('get_best_matches: one group id per candidate')
    q = PackedSpectra.from_spectra([query])
    lib = PackedSpectra.from_spectra(candidates)
    offsets = np.array([0, len(candidates)], np.int32)
    rows = np.arange(len(candidates), dtype=np.int64)
    best, score, counts, pairs = rescore_batch_topn(q, lib, rows, offsets, fragment_mz_tolerance,
                                                    allow_shift, n, groups=groups,
                                                    fragment_tolerance_unit=fragment_tolerance_unit)
    return [(candidates[int(best[0, r])], float(score[0, r]),
             [(int(a), int(b)) for a, b in pairs[0, r, :int(counts[0, r])]])
            for r in range(best.shape[1]) if best[0, r] >= 0]


def rescore_batch(queries: PackedSpectra, library: PackedSpectra, cand_rows, cand_offsets,
                  fragment_mz_tolerance, allow_shift, pm_stride=None, fragment_tolerance_unit='Da'):
    """Batched ``get_best_match``: candidates of query q are
    ``cand_rows[cand_offsets[q]:cand_offsets[q+1]]`` (library rows). Returns numpy
    ``(best_cand[nq], best_score[nq], pm_count[nq], pm_pairs[nq, pm_stride, 2])``."""
    flags = score_flags(allow_shift, fragment_tolerance_unit)
    nq = queries.n
    if pm_stride is None:
        cnt = np.diff(np.asarray(queries.offsets.cpu()))
        pm_stride = int(cnt.max()) if nq else 1
    cand_rows = np.ascontiguousarray(cand_rows, np.int64) if isinstance(
        cand_rows, (list, np.ndarray)) else cand_rows
    cand_offsets = np.ascontiguousarray(cand_offsets, np.int32) if isinstance(
        cand_offsets, (list, np.ndarray)) else cand_offsets
    best = np.empty(nq, np.int32)
    score = np.empty(nq, np.float64)
    count = np.empty(nq, np.int32)
    pairs = np.zeros((nq, pm_stride, 2), np.uint32)
    qs, ls = _lib.peaks_struct(queries), _lib.peaks_struct(library)
    _lib.check(_lib.lib().asl_rescore_batch(
        qs, ls, _lib.ptr(cand_rows), _lib.ptr(cand_offsets), float(fragment_mz_tolerance),
        flags, _lib.ptr(best), _lib.ptr(score), _lib.ptr(count),
        _lib.ptr(pairs), pm_stride))
    return best, score, count, pairs


def rescore_batch_topn(queries: PackedSpectra, library: PackedSpectra, cand_rows, cand_offsets,
                       fragment_mz_tolerance, allow_shift, n_best, pm_stride=None, groups=None,
                       fragment_tolerance_unit='Da'):
    """``rescore_batch`` for the ``n_best`` (1 .. 16) best candidates of every query, ordered by
    score descending, equal scores by position in the query's list. Returns numpy
    ``(best_cand[nq, n], best_score[nq, n], pm_count[nq, n], pm_pairs[nq, n, pm_stride, 2])``;
    ranks beyond a list's valid entries hold -1 / 0.0 / 0 / zeros. ``groups`` (int32 per LIBRARY row,
    numpy or device tensor): distinct ranks -- a slot is skipped when an earlier rank holds a row of
    its group, negative ids never collide (``asl_rescore_batch_topn_distinct``)."""
    flags = score_flags(allow_shift, fragment_tolerance_unit)
    nq, n = queries.n, int(n_best)
    if pm_stride is None:
        cnt = np.diff(np.asarray(queries.offsets.cpu()))
        pm_stride = int(cnt.max()) if nq else 1
    cand_rows = np.ascontiguousarray(cand_rows, np.int64) if isinstance(
        cand_rows, (list, np.ndarray)) else cand_rows
    cand_offsets = np.ascontiguousarray(cand_offsets, np.int32) if isinstance(
        cand_offsets, (list, np.ndarray)) else cand_offsets
    shape = (nq, max(n, 0))
    best = np.empty(shape, np.int32)
    score = np.empty(shape, np.float64)
    count = np.empty(shape, np.int32)
    pairs = np.zeros(shape + (pm_stride, 2), np.uint32)
    qs, ls = _lib.peaks_struct(queries), _lib.peaks_struct(library)
    if groups is not None:
        if isinstance(groups, (list, tuple, np.ndarray)):
            groups = np.ascontiguousarray(groups, np.int32)
        if len(groups) != library.n:
            raise ValueError('rescore_batch_topn: one group id per library row')
        _lib.check(_lib.lib().asl_rescore_batch_topn_distinct(
            qs, ls, _lib.ptr(cand_rows), _lib.ptr(cand_offsets), _lib.ptr(groups),
            float(fragment_mz_tolerance), flags, n, _lib.ptr(best), _lib.ptr(score),
            _lib.ptr(count), _lib.ptr(pairs), pm_stride))
        return best, score, count, pairs
    _lib.check(_lib.lib().asl_rescore_batch_topn(
        qs, ls, _lib.ptr(cand_rows), _lib.ptr(cand_offsets), float(fragment_mz_tolerance),
        flags, n, _lib.ptr(best), _lib.ptr(score), _lib.ptr(count),
        _lib.ptr(pairs), pm_stride))
    return best, score, count, pairs
