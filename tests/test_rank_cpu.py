"""asl_index_rank without a GPU: the export, ASL_ERR_NO_DEVICE, and the expected-rank helper the GPU
tests lean on, against a ranking made by hand."""
import numpy as np
import pytest

from rank_ref import expected_ranks, neighbour_order, rank_in_row


def _has_device():
    from ann_solo_amd import _lib
    return _lib.lib().asl_get_num_gpus() > 0


def test_symbol_is_exported():
    from ann_solo_amd import _lib
    assert 'asl_index_rank' in _lib.EXPORTS
    assert hasattr(_lib.lib(), 'asl_index_rank')
    from ann_solo_amd import faiss_compat
    from ann_solo_amd.spectral_library import SpectralLibrary
    assert callable(faiss_compat.IndexIVFFlat.rank_of) and callable(faiss_compat.IndexIVFPQ.rank_of)
    assert callable(SpectralLibrary.candidate_rank)


@pytest.mark.skipif(_has_device(), reason='checks the behaviour without a HIP device')
def test_rank_needs_a_device():
    from ann_solo_amd import _lib
    x = np.zeros((1, 800), np.float32)
    t = np.zeros(1, np.int64)
    r = np.zeros(1, np.int64)
    assert _lib.lib().asl_index_rank(None, 1, _lib.ptr(x), _lib.ptr(t), 0, None, None, 2, 0.0, 0, _lib.ptr(r),
                                     None, None) == -2          # ASL_ERR_NO_DEVICE


def test_helper_on_ten_vectors_with_ties():
    #        id:   0    1    2    3    4    5    6    7    8    9
    scores = [0.5, 0.9, 0.5, 0.0, 0.9, 0.2, 0.5, 0.0, 1.0, 0.2]
    ids = np.arange(10)
    order = neighbour_order(scores, ids)
    # by hand: 1.0 -> 8; 0.9 -> 1, 4; 0.5 -> 0, 2, 6; 0.2 -> 5, 9; 0.0 -> 3, 7 (ties by ascending id)
    assert order.tolist() == [8, 1, 4, 0, 2, 6, 5, 9, 3, 7]
    by_hand = {8: 0, 1: 1, 4: 2, 0: 3, 2: 4, 6: 5, 5: 6, 9: 7, 3: 8, 7: 9}
    for t, r in by_hand.items():
        assert rank_in_row(order, t) == r
        # the definition: the number of vectors whose key beats the target's
        s = np.asarray(scores, np.float32)
        assert r == int(((s > s[t]) | ((s == s[t]) & (ids < t))).sum())
    assert rank_in_row(order, -1) == -1 and rank_in_row(order, 10) == -1
    # a scope that lacks some vectors (lists not probed): -1 padded rows, ranks among what is there
    part = np.array([8, 4, 0, 6, 9, 7, -1, -1, -1, -1])
    rows = np.stack([order, part, part])
    assert expected_ranks(rows, [6, 6, 1]).tolist() == [5, 3, -1]
    # ids that are not 0..n-1, given in any order
    assert neighbour_order([0.1, 0.7, 0.7, 0.1], [40, 30, 20, 10]).tolist() == [20, 30, 10, 40]
