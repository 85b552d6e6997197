"""Subset search, the parts that need no GPU: the reference of tests/selector_ref.py checks itself, the
inputs of the GPU tests have the properties those tests rely on, and ``set_search_subset`` checks its
arguments."""
from types import SimpleNamespace

import numpy as np
import pytest

import selector_ref as R

K, NPROBE, NLIST, NQ = 256, 8, 16, 48


@pytest.fixture(scope='module')
def world(O):
    from ann_solo_amd import synthetic
    lib, aux = synthetic.make_library(5000, seed=71, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, NQ, seed=72, charge=2)
    o, mz, it, *_ = lib.numpy()
    qo, qmz, qit, *_ = q.numpy()
    _, min_bound, _ = O.get_dim(11, 2010, 0.04)
    xb = O.encode_batch(mz, it, o, min_bound, 0.04, 800)
    xq = O.encode_batch(qmz, qit, qo, min_bound, 0.04, 800)
    cen = O.kmeans(xb, NLIST, niter=4, seed=1234)
    ivf = O.HostIVF(cen, O.assign(xb, cen), xb)
    return ivf, xq, len(xb), ivf.search(xq, K, NPROBE)


def _masks(n):
    ids = np.arange(n)
    return dict(every3=ids % 3 == 0, every16=ids % 16 == 0, rand30=np.random.default_rng(1).random(n) < 0.3,
                all=np.ones(n, bool), none=np.zeros(n, bool))


@pytest.mark.parametrize('name', ['every3', 'every16', 'rand30', 'all', 'none'])
def test_reference_agrees_with_search_all_then_select(O, world, name):
    ivf, xq, n, _ = world
    keep = _masks(n)[name]
    got = R.search_selected(O, ivf, xq, K, NPROBE, keep)
    want = R.search_all_then_select(O, ivf, xq, K, NPROBE, keep)
    R.assert_rows_equal(got, want, name)
    ids = got[1][got[1] >= 0]
    assert keep[ids].all()


def test_conditions_the_gpu_tests_rely_on(O, world):
    ivf, xq, n, (D0, I0) = world
    m = _masks(n)
    # every third id: every row is full, and holds strictly more than the plain row filtered afterwards
    _, I3 = R.search_selected(O, ivf, xq, K, NPROBE, m['every3'])
    assert int((I3 >= 0).all(1).sum()) == NQ
    post = R.post_filtered(I0, m['every3'])
    for i in range(NQ):
        assert set(post[i].tolist()) < set(I3[i].tolist()), i
    # every sixteenth id: every row is short
    _, I16 = R.search_selected(O, ivf, xq, K, NPROBE, m['every16'])
    assert int((I16 < 0).any(1).sum()) == NQ
    assert (I16[:, 0] >= 0).all()
    # all selected: the plain rows; none: nothing
    R.assert_rows_equal(R.search_selected(O, ivf, xq, K, NPROBE, m['all']), (D0, I0))
    assert (R.search_selected(O, ivf, xq, K, NPROBE, m['none'])[1] == -1).all()


def test_key_with_selection():
    key = np.array([1.0, 2.0, np.nan, 4.0], np.float32)
    out = R.key_with_selection(key, [True, False, True, True])
    assert out.dtype == np.float32 and np.array_equal(np.isnan(out), [False, True, True, False])
    assert out[0] == 1.0 and out[3] == 4.0 and not np.isnan(key[1])


def _bare_library(sizes):
    from ann_solo_amd.spectral_library import SpectralLibrary
    sl = SpectralLibrary.__new__(SpectralLibrary)
    sl.partitions = {z: SimpleNamespace(ids=np.arange(n), handle=None) for z, n in sizes.items()}
    sl._dist = None
    return sl


def test_set_search_subset_checks_its_arguments():
    sl = _bare_library({2: 10, 3: 7})
    with pytest.raises(ValueError, match=r'charge\(s\) \[3\]'):
        sl.set_search_subset({2: np.ones(10, bool)})
    with pytest.raises(ValueError, match='flags for the 7 rows'):
        sl.set_search_subset({2: np.ones(10, bool), 3: np.ones(8, bool)})
    with pytest.raises(ValueError, match='flags for the 10 rows'):
        sl.set_search_subset({2: np.ones((10, 1), bool), 3: np.ones(7, bool)})
    sl._dist = SimpleNamespace(world=2)
    with pytest.raises(ValueError, match='sharded'):
        sl.set_search_subset({2: np.ones(10, bool), 3: np.ones(7, bool)})
