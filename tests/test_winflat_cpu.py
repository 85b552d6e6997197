"""The window-exact index without a GPU: its reference (tests/winflat_ref.py) agrees with itself, and the
configuration layer accepts `index = 'winflat'` and refuses what the index does not serve."""
import argparse

import numpy as np
import pytest

import winflat_ref as WR


def _vectors(n, d, nnz, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, d), np.float32)
    for i in range(n):
        x[i, rng.choice(d, nnz, replace=False)] = rng.random(nnz).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[n // 3] = x[0]                      # a score tie: the lower id first
    return x


def test_reference_agrees_with_itself(O):
    xb, xq = _vectors(700, 96, 6, 1), _vectors(9, 96, 6, 2)
    key = (400 + 0.5 * np.random.default_rng(3).permutation(len(xb))).astype(np.float32)
    key[::11] = np.nan
    q_pmz = np.linspace(420.0, 700.0, len(xq))
    for i in range(0, len(xb), 37):       # the vectorised masks are precursor_ok
        for tol, mode in ((30.0, 'Da'), (5e4, 'ppm')):
            assert bool(WR.mask(q_pmz[1], key[i:i + 1], 2, tol, mode)[0]) == O.precursor_ok(q_pmz[1], key[i], 2, tol, mode)
    assert not WR.interval_mask(np.nan, 500.0, key).any() and not WR.interval_mask(500.0, 400.0, key).any()
    assert WR.interval_mask(-np.inf, np.inf, key).sum() == np.isfinite(key).sum()
    assert np.array_equal(WR.interval_mask(410.0, 415.0, key), (key >= 410.0) & (key <= 415.0))
    for k in (5, 40):
        keeps = [WR.mask(q_pmz[i], key, 2, 30.0, 'Da') for i in range(len(xq))]
        D, I = WR.search(O, xb, xq, k, keeps)
        for i in range(len(xq)):          # the one-list HostIVF search is the flat search over the kept vectors
            rD, rI = WR.one_list_ivf(O, xb, keeps[i]).search(xq[i:i + 1], k, 1)
            assert np.array_equal(I[i], rI[0])
            v = rI[0] >= 0
            assert np.array_equal(D[i][v].view(np.uint32), rD[0][v].view(np.uint32))
            assert keeps[i][I[i][v]].all()
        everything = [np.ones(len(xb), bool)] * len(xq)      # an all-passing window is the plain search
        D, I = WR.search(O, xb, xq, k, everything)
        fD, fI = O.flat_search(xb, xq, k)
        assert np.array_equal(I, fI) and np.array_equal(D.view(np.uint32), fD.view(np.uint32))
    _, I = WR.search(O, xb, xb[:1], 2, [np.ones(len(xb), bool)])
    assert I[0].tolist() == [0, len(xb) // 3]


def test_config_accepts_winflat_and_refuses_what_it_does_not_serve():
    from ann_solo_amd.config import Config
    cfg = Config.open_search(index='winflat', num_candidates=256)
    assert cfg.index == 'winflat' and cfg.ann_window == 'post'
    assert Config(index='winflat', flat_storage='fx22').flat_storage == 'fx22'
    for bad in (dict(num_gpus=2), dict(refine_k=512), dict(ann_window='pre'), dict(pq_by_residual=False),
                dict(num_candidates=1281)):
        with pytest.raises(ValueError):
            Config.open_search(index='winflat', **bad)


def test_add_arguments_parses_winflat():
    from ann_solo_amd.config import Config, add_arguments
    p = argparse.ArgumentParser()
    add_arguments(p)
    ns = p.parse_args(['--index', 'winflat'])
    assert ns.index == 'winflat'
    assert Config.from_reference(ns).index == 'winflat'
    with pytest.raises(SystemExit):
        p.parse_args(['--index', 'winflat2'])
