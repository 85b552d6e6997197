"""`Config.ann_window` and the window-scan entry points without a GPU: the flag, its validation, the
index-file hashes it must not touch, and ASL_ERR_NO_DEVICE from the new compute entry points."""
import argparse

import numpy as np
import pytest

from ann_solo_amd.config import Config, add_arguments


def _has_device():
    from ann_solo_amd import _lib
    return _lib.lib().asl_get_num_gpus() > 0


def test_flag_parsing_and_default():
    assert Config().ann_window == 'post'
    p = argparse.ArgumentParser()
    add_arguments(p)
    assert p.parse_args([]).ann_window == 'post'
    ns = p.parse_args(['--ann_window', 'pre', '--index', 'ivfpq'])
    assert ns.ann_window == 'pre'
    assert Config.from_reference(ns).ann_window == 'pre'
    with pytest.raises(SystemExit):
        p.parse_args(['--ann_window', 'inside'])


def test_validation_errors():
    assert Config(index='ivfpq', ann_window='pre').ann_window == 'pre'
    with pytest.raises(ValueError):
        Config(ann_window='inside')
    with pytest.raises(ValueError):
        Config(ann_window='pre')                          # the default index is IVF-Flat
    with pytest.raises(ValueError):
        Config(index='ivfflat', ann_window='pre')
    with pytest.raises(ValueError):
        Config(index='ivfpq', pq_m=16, ann_window='pre')  # the generic PQ kernel
    with pytest.raises(ValueError):
        Config(index='ivfpq', num_gpus=2, ann_window='pre')
    with pytest.raises(ValueError):
        Config(index='ivfpq', refine_k=512, ann_window='pre')
    Config(index='ivfpq', num_gpus=2, refine_k=512)       # 'post' keeps every combination


def test_hashes_do_not_depend_on_ann_window():
    from ann_solo_amd.spectral_library import SpectralLibrary
    out = {}
    for w in ('post', 'pre'):
        sl = SpectralLibrary.__new__(SpectralLibrary)
        sl.config = Config.open_search(index='ivfpq', ann_window=w)
        out[w] = (sl._get_hyperparameter_hash(), sl._get_index_hash())
    assert out['post'] == out['pre']


@pytest.mark.skipif(_has_device(), reason='checks the behaviour without a HIP device')
def test_compute_entry_points_need_a_device():
    from ann_solo_amd import _lib
    L = _lib.lib()
    key = np.zeros(4, np.float32)
    x = np.zeros((1, 800), np.float32)
    pmz = np.zeros(1, np.float64)
    D = np.zeros((1, 4), np.float32)
    I = np.zeros((1, 4), np.int64)
    assert L.asl_index_set_window_key(None, 4, _lib.ptr(key)) == -2           # ASL_ERR_NO_DEVICE
    assert L.asl_index_search_window(None, 1, _lib.ptr(x), _lib.ptr(pmz), 2, 500.0, 0, 4, 8,
                                     _lib.ptr(D), _lib.ptr(I)) == -2
    assert L.asl_index_set_window_scan(None, 1) == -1                        # a setter: the null handle
