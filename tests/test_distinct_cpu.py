"""`Config.distinct_matches` and the distinct top-n entry points without a GPU: the flag, its
validation, the index-file hashes it must not touch, the reference rule on hand-made lists, the four
exports, and ASL_ERR_NO_DEVICE / ASL_ERR_INVALID from the compute entry points."""
import argparse

import numpy as np
import pytest

from ann_solo_amd.config import Config, add_arguments
from distinct_ref import distinct_select, oracle_ranks_distinct

DISTINCT = ('asl_library_set_groups', 'asl_rescore_batch_topn_distinct', 'asl_search_batch_topn_distinct',
            'asl_rescore_knn_topn_distinct')


def _has_device():
    from ann_solo_amd import _lib
    return _lib.lib().asl_get_num_gpus() > 0


def test_flag_parsing_and_default():
    assert Config().distinct_matches is False
    p = argparse.ArgumentParser()
    add_arguments(p)
    assert p.parse_args([]).distinct_matches is False
    ns = p.parse_args(['--num_matches', '5', '--distinct_matches'])
    assert ns.distinct_matches is True
    cfg = Config.from_reference(ns)
    assert cfg.distinct_matches is True and cfg.num_matches == 5
    with pytest.raises(SystemExit):
        p.parse_args(['--distinct_matches', 'yes'])           # a switch: it takes no value


def test_validation_errors():
    assert Config(num_matches=16, distinct_matches=True).distinct_matches
    assert Config(distinct_matches=True).num_matches == 1     # harmless alone: one rank is one group
    assert Config(num_gpus=1, num_matches=3, distinct_matches=True).distinct_matches
    with pytest.raises(ValueError):
        Config(distinct_matches=True, num_gpus=2)
    with pytest.raises(ValueError):
        Config.open_search(index='ivfpq', distinct_matches=True, num_gpus=4)
    with pytest.raises(ValueError):
        Config.from_reference(argparse.Namespace(distinct_matches=True, num_gpus=2))


def test_hashes_do_not_depend_on_distinct_matches():
    from ann_solo_amd.spectral_library import SpectralLibrary
    out = {}
    for flag in (False, True):
        for index in ('ivfflat', 'ivfpq'):
            sl = SpectralLibrary.__new__(SpectralLibrary)
            sl.config = Config.open_search(index=index, num_matches=5, distinct_matches=flag)
            out[flag, index] = (sl._get_hyperparameter_hash(), sl._get_index_hash())
    for index in ('ivfflat', 'ivfpq'):
        assert out[False, index] == out[True, index]


def test_rule_on_hand_made_lists():
    #            pos:  0    1    2    3    4    5     6    7
    score = np.array([0.5, 0.9, 0.9, 0.7, -1.0, 0.7, 0.2, 0.9])
    key = np.array([10, 7, 3, 4, 0, 4, 1, 3])              # 2 and 7: the same row listed twice
    one = np.zeros(8, int)
    assert distinct_select(score, key, np.full(8, -1), 3) == [2, 7, 1]      # ungrouped: the plain ranks
    assert distinct_select(score, key, np.full(8, -1), 16) == [2, 7, 1, 3, 5, 0, 6]
    assert distinct_select(score, key, one, 5) == [2]                        # one group: rank 0 only
    grp = np.array([0, 1, 1, 2, 9, 0, 3, 1])
    assert distinct_select(score, key, grp, 16) == [2, 3, 5, 6]              # 5 (group 0) beats 0 on score
    grp = np.array([0, 1, 1, 2, 9, 5, 3, 1])
    assert distinct_select(score, key, grp, 16) == [2, 3, 5, 0, 6]
    assert distinct_select(score, key, grp, 2) == [2, 3]
    # a row listed twice and ungrouped takes two ranks; grouped, one
    grp = np.array([0, 1, -1, 2, 9, 5, 3, -1])
    assert distinct_select(score, key, grp, 4) == [2, 7, 1, 3]
    assert distinct_select(np.full(4, -1.0), np.arange(4), np.arange(4), 3) == []
    assert distinct_select([], [], [], 3) == []


class _FakeOracle:
    """best_match over given scores: the first strict maximum (SpectrumMatch.cpp:118-129)."""
    def __init__(self, score_of_row):
        self.score_of_row = np.asarray(score_of_row, np.float64)

    def best_match(self, Q, i, L, cand, tol, shift):
        s = self.score_of_row[cand]
        b = int(np.argmax(s))                                 # argmax: the first of equal maxima
        return b, float(s[b]), np.zeros((0, 2), np.int64)


def test_delete_the_group_rule_equals_the_walk():
    rng = np.random.default_rng(3)
    for trial in range(200):
        n_lib = int(rng.integers(1, 40))
        score_of_row = rng.integers(0, 6, n_lib) / 4.0        # many ties
        row_group = rng.integers(-1, 5, n_lib)
        cand = rng.integers(0, n_lib, int(rng.integers(0, 30)))          # caller order, rows repeat
        O = _FakeOracle(score_of_row)
        for n in (1, 2, 5, 16):
            got = oracle_ranks_distinct(O, None, 0, None, cand, row_group, n)
            # on a caller-ordered list "first strict maximum" is "ties to the earlier position"
            want = distinct_select(score_of_row[cand], np.arange(len(cand)), row_group[cand], n)
            assert [p for p, _, _, _ in got] == want, (trial, n)
            rows = [r for _, r, _, _ in got]
            g = row_group[rows]
            assert len(set(g[g >= 0])) == (g >= 0).sum()                 # one rank per group
        # ascending rows: "first strict maximum" is "ties to the lower row"
        asc = np.unique(cand)
        got = oracle_ranks_distinct(O, None, 0, None, asc, row_group, 16)
        assert [p for p, _, _, _ in got] == distinct_select(score_of_row[asc], asc, row_group[asc], 16)


def test_exports():
    from ann_solo_amd import _lib
    L = _lib.lib()
    for name in DISTINCT:
        assert name in _lib.EXPORTS and hasattr(L, name)
    import os
    header = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'annsolo_mi.h')).read()
    for name in DISTINCT:
        assert name + '(' in header


@pytest.mark.skipif(_has_device(), reason='checks the behaviour without a HIP device')
def test_compute_entry_points_need_a_device():
    from ann_solo_amd import _lib
    L = _lib.lib()
    assert L.asl_rescore_batch_topn_distinct(None, None, None, None, None, 0.02, 1, 2, None, None, None, None,
                                             0) == -2
    assert L.asl_search_batch_topn_distinct(None, None, None, None, 3, None, None, None, None, None, 0,
                                            None) == -2
    assert L.asl_rescore_knn_topn_distinct(None, None, None, None, 16, None, None, None, None, None, 0) == -2
    # the rank count is checked before anything touches the device
    for bad in (0, 17, -1):
        assert L.asl_rescore_batch_topn_distinct(None, None, None, None, None, 0.02, 1, bad, None, None, None,
                                                 None, 0) == -1
        assert b'n_best' in L.asl_last_error()
        assert L.asl_search_batch_topn_distinct(None, None, None, None, bad, None, None, None, None, None, 0,
                                                None) == -1
        assert b'n_best' in L.asl_last_error()
        assert L.asl_rescore_knn_topn_distinct(None, None, None, None, bad, None, None, None, None, None,
                                               0) == -1
        assert b'n_best' in L.asl_last_error()
    assert L.asl_library_set_groups(None, 0, None) == -1      # no handle: nothing to set


def test_get_best_matches_checks_the_groups():
    from ann_solo_amd.spectrum_match import get_best_matches
    with pytest.raises(ValueError):
        get_best_matches(object(), [], 0.02, True, 3, groups=[])
    with pytest.raises(ValueError):
        get_best_matches(object(), [object(), object()], 0.02, True, 3, groups=[1])
