"""`Config.num_matches` and the top-n entry points without a GPU: the flag, its validation, the
index-file hashes it must not touch, ASL_ERR_NO_DEVICE from the three compute entry points, and the
SSM record's new fields."""
import argparse

import numpy as np
import pytest

from ann_solo_amd.config import Config, add_arguments


def _has_device():
    from ann_solo_amd import _lib
    return _lib.lib().asl_get_num_gpus() > 0


def test_flag_parsing_and_default():
    assert Config().num_matches == 1
    p = argparse.ArgumentParser()
    add_arguments(p)
    assert p.parse_args([]).num_matches == 1
    ns = p.parse_args(['--num_matches', '5'])
    assert ns.num_matches == 5
    assert Config.from_reference(ns).num_matches == 5
    with pytest.raises(SystemExit):
        p.parse_args(['--num_matches', 'many'])


def test_validation_errors():
    assert Config(num_matches=16).num_matches == 16
    assert Config(num_matches=1, num_gpus=2).num_matches == 1
    for bad in (0, 17, -3):
        with pytest.raises(ValueError):
            Config(num_matches=bad)
    with pytest.raises(ValueError):
        Config(num_matches=2, num_gpus=2)
    with pytest.raises(ValueError):
        Config.open_search(index='ivfpq', num_matches=3, num_gpus=4)
    with pytest.raises(ValueError):
        Config.from_reference(argparse.Namespace(num_matches=17))


def test_hashes_do_not_depend_on_num_matches():
    from ann_solo_amd.spectral_library import SpectralLibrary
    out = {}
    for n in (1, 5):
        for index in ('ivfflat', 'ivfpq'):
            sl = SpectralLibrary.__new__(SpectralLibrary)
            sl.config = Config.open_search(index=index, num_matches=n)
            out[n, index] = (sl._get_hyperparameter_hash(), sl._get_index_hash())
    for index in ('ivfflat', 'ivfpq'):
        assert out[1, index] == out[5, index]


def test_exports_and_limit():
    from ann_solo_amd import _lib
    L = _lib.lib()
    for name in ('asl_rescore_batch_topn', 'asl_search_batch_topn', 'asl_rescore_knn_topn'):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert Config.MAX_MATCHES == 16


@pytest.mark.skipif(_has_device(), reason='checks the behaviour without a HIP device')
def test_compute_entry_points_need_a_device():
    from ann_solo_amd import _lib
    L = _lib.lib()
    assert L.asl_rescore_batch_topn(None, None, None, None, 0.02, 1, 2, None, None, None, None, 0) == -2
    assert L.asl_search_batch_topn(None, None, None, None, 3, None, None, None, None, None, 0, None) == -2
    assert L.asl_rescore_knn_topn(None, None, None, None, 16, None, None, None, None, None, 0) == -2
    # the rank count is checked before anything touches the device
    assert L.asl_search_batch_topn(None, None, None, None, 0, None, None, None, None, None, 0, None) == -1
    assert b'n_best' in L.asl_last_error()
    assert L.asl_rescore_knn_topn(None, None, None, None, 17, None, None, None, None, None, 0) == -1


def test_get_best_matches_needs_a_candidate():
    from ann_solo_amd.spectrum_match import get_best_match, get_best_matches
    with pytest.raises(ValueError):
        get_best_match(object(), [], 0.02, True)
    with pytest.raises(ValueError):
        get_best_matches(object(), [], 0.02, True, 3)


def test_ssm_record_fields_default():
    from ann_solo_amd.spectrum import SpectrumSpectrumMatch
    old = SpectrumSpectrumMatch('PEPTIDE', 'q1', 0, 7, 1.0, 2, 500.0, 499.9, False, 0.5, 0.0, np.zeros((0, 2)))
    assert np.isnan(old.delta_score) and old.alternatives == ()
    new = SpectrumSpectrumMatch('PEPTIDE', 'q1', 0, 7, 1.0, 2, 500.0, 499.9, False, 0.5, 0.0, np.zeros((0, 2)),
                                0.25, ((8, 0.25, np.zeros((0, 2))),))
    assert new.delta_score == 0.25 and new.alternatives[0][0] == 8


def test_ssm_table_carries_the_alternatives():
    from types import SimpleNamespace
    from ann_solo_amd.spectral_library import BatchResult, SSMTable, TopnBatchResult
    rows = np.array([[4, 2, -1], [-1, -1, -1], [1, 3, 0]], np.int32)
    scores = np.array([[0.9, 0.5, 0.0], [0.0, 0.0, 0.0], [0.75, 0.75, 0.25]])
    cnt = np.array([[2, 1, 0], [0, 0, 0], [1, 1, 1]], np.int32)
    pairs = np.zeros((3, 3, 4, 2), np.uint32)
    pairs[0, 1, 0] = (3, 1)
    pairs[2, 2, 0] = (2, 2)
    top = TopnBatchResult(rows, scores, np.array([5, 0, 3], np.int32), cnt, pairs)
    res = top.rank0()
    assert isinstance(res, BatchResult) and np.array_equal(res.best_row, rows[:, 0])
    res.topn = top
    meta = {2: [dict(identifier=i, peptide='P%d' % i, precursor_mz=500.0 + i, index=i, precursor_charge=2)
                for i in range(5)]}
    t = SSMTable(meta, meta, 2)
    t.add_batch(2, np.array([10, 11, 12]) % 5, res.best_row, np.array([0.1, 0.2, 0.3]), res)
    assert len(t) == 2                                  # the query without a candidate has no SSM
    assert np.array_equal(t.alt_lib_row, [[2, -1], [3, 0]])
    assert np.array_equal(t.alt_score, [[0.5, 0.0], [0.75, 0.25]])
    assert t.delta_score[0] == 0.9 - 0.5 and t.delta_score[1] == 0.0
    assert np.array_equal(t.alt_peak_matches(0, 1), [[3, 1]]) and len(t.alt_peak_matches(0, 2)) == 0
    assert np.array_equal(t.alt_peak_matches(1, 2), [[2, 2]])
    with pytest.raises(IndexError):
        t.alt_peak_matches(0, 3)
    t.q[:] = 0.0
    rec = t[1]
    assert rec.delta_score == 0.0 and [a[0] for a in rec.alternatives] == [3, 0]
    assert rec.alternatives[0][1] == 0.75 and np.array_equal(rec.alternatives[1][2], [[2, 2]])
    sub = t.take(np.array([False, True]))
    assert np.array_equal(sub.alt_lib_row, [[3, 0]]) and np.array_equal(sub.alt_peak_matches(0, 2), [[2, 2]])
    both = SSMTable.concat([sub, t])
    assert len(both) == 3 and np.array_equal(both.alt_lib_row[:, 0], [3, 2, 3])
    assert np.array_equal(both.alt_peak_matches(1, 1), [[3, 1]])
    plain = SSMTable(meta, meta)                       # num_matches = 1: no alternatives, no gap
    single = BatchResult(rows[:, 0].copy(), scores[:, 0].copy(), top.n_candidates, cnt[:, 0].copy(),
                         pairs[:, 0].copy())
    plain.add_batch(2, np.array([0, 1, 2]), single.best_row, np.array([0.1, 0.2, 0.3]), single)
    assert plain.alt_lib_row.shape == (2, 0) and np.isnan(plain.delta_score).all()
    plain.q[:] = 0.0
    assert plain[0].alternatives == () and np.isnan(plain[0].delta_score)
    del SimpleNamespace
