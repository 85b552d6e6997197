"""IVF-PQ on the raw vectors (FAISS' ``by_residual = false``) without a GPU: the reference the GPU
tests compare against is the oracle's own arithmetic, the configuration flag, the cache-file hashes
it must not move, and the two new entry points of the C ABI."""
import argparse
import hashlib
import json
import os
import re

import numpy as np
import pytest

import raw_pq_ref as R
from ann_solo_amd.config import Config, add_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('m', [32, 16, 64, 4])
def test_numpy_adc_tree_is_the_oracles(O, m):
    """``adc_tree`` against ``O.adc(lut, code, 0.0)`` on 200 codes, uint32 bits (m = 4: partials with no
    sub-quantiser are the oracle's 0.0f)."""
    rng = np.random.default_rng(m)
    lut = rng.standard_normal((m, 256)).astype(np.float32)
    lut[:, :3] = 0.0
    codes = rng.integers(0, 256, (200, m)).astype(np.uint8)
    codes[:5] = 0                                         # all-zero sums: 0.0f + 0.0f
    want = np.array([O.adc(lut, c, 0.0) for c in codes], np.float32)
    got = R.adc_tree(lut, codes)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and the coarse term does matter to the bits: the by-residual score of the same codes differs
    other = np.array([O.adc(lut, c, 0.37) for c in codes], np.float32)
    assert (other.view(np.uint32) != want.view(np.uint32)).any()


def test_a_zero_centroid_makes_the_oracle_quantise_the_vectors(O):
    """The residual against one all-zero centroid is the vector: codes are the nearest codebook entry of
    the raw sub-vector (ties: the lowest code), checked in float64 where the margin is clear."""
    rng = np.random.default_rng(3)
    x = (rng.random((600, 32)) * (rng.random((600, 32)) < 0.2)).astype(np.float32)
    cb, codes = R.raw_quantiser(O, x, 4, 16, 3, 99)
    assert cb.shape == (4, 16, 8) and codes.shape == (600, 4)
    sub = x.reshape(600, 4, 8).astype(np.float64)
    d2 = ((sub[:, :, None, :] - cb[None].astype(np.float64)) ** 2).sum(-1)      # [n, m, ksub]
    best = d2.min(-1)
    assert np.all(np.take_along_axis(d2, codes[..., None].astype(np.int64), -1)[..., 0] <= best * (1 + 1e-5) + 1e-12)
    assert np.array_equal(codes, R.raw_codes(O, x, cb))


def test_raw_search_is_the_oracles_adc_over_the_probed_lists(O):
    """``raw_search`` against a plain loop: every vector of every probed list scored by ``O.adc(lut, code, 0.0)``,
    sorted (score desc, id asc); with a keep-mask, the kept vectors only."""
    rng = np.random.default_rng(11)
    x = (rng.random((700, 32)) * (rng.random((700, 32)) < 0.3)).astype(np.float32)
    x[600:650] = x[5]
    xq = x[[5, 17, 300]].copy()
    xq[2] = 0.0
    cen = O.kmeans(x, 4, 2, 77, 0, 256)
    a = O.assign(x, cen, 0)
    cb, codes = R.raw_quantiser(O, x, 4, 16, 2, 84)
    ivf = O.HostIVF(cen, a, codes, cb)
    keep = rng.random((3, 700)) < 0.5
    _, cI = O.coarse(xq, cen, 2)
    for mask in (None, keep):
        D, I = R.raw_search(O, xq, cen, ivf, 400, 2, keep=mask)
        for q in range(3):
            lut = O.pq_lut(xq[q], cb)
            hits = [(-np.float32(O.adc(lut, ivf.payload[p], 0.0)), int(ivf.ids[p]))
                    for l in cI[q] for p in range(ivf.list_offsets[l], ivf.list_offsets[l + 1])
                    if mask is None or mask[q, ivf.ids[p]]]
            hits.sort()
            hits = hits[:400]
            n = len(hits)
            assert I[q, :n].tolist() == [h[1] for h in hits] and (I[q, n:] == -1).all()
            assert np.array_equal(D[q, :n].view(np.uint32), np.array([-h[0] for h in hits], np.float32).view(np.uint32))
            assert (D[q, n:] == R.PAD_D).all()
    assert (I == -1).any() and len(set(D[2][I[2] >= 0].tolist())) == 1        # padded rows; the all-zero query ties


def test_rank_pads_and_breaks_ties_by_id():
    D, I = R._rank(np.array([1.0, 2.0, 1.0, 2.0], np.float32), np.array([9, 4, 3, 8], np.int64), 6)
    assert I.tolist() == [4, 8, 3, 9, -1, -1]
    assert D[:4].tolist() == [2.0, 2.0, 1.0, 1.0] and (D[4:] == R.PAD_D).all() and R.PAD_D == -np.finfo(np.float32).max


def test_flag_parsing_defaults_and_validation():
    assert Config().pq_by_residual is True
    assert Config.open_search(index='ivfpq').pq_by_residual is True
    p = argparse.ArgumentParser()
    add_arguments(p)
    assert p.parse_args([]).pq_by_residual == 1
    assert Config.from_reference(p.parse_args([])).pq_by_residual is True
    ns = p.parse_args(['--index', 'ivfpq', '--pq_by_residual', '0'])
    assert ns.pq_by_residual == 0
    assert Config.from_reference(ns).pq_by_residual is False
    assert Config.from_reference(p.parse_args(['--pq_by_residual', '1'])).pq_by_residual is True
    with pytest.raises(SystemExit):
        p.parse_args(['--pq_by_residual', '2'])
    with pytest.raises(ValueError):
        Config(pq_by_residual=False)                      # the default index is IVF-Flat
    with pytest.raises(ValueError):
        Config(index='ivfflat', pq_by_residual=False)
    with pytest.raises(ValueError):
        Config.from_reference(p.parse_args(['--pq_by_residual', '0']))
    # every combination IVF-PQ has stays legal with raw codes
    for kw in (dict(refine_k=2048), dict(num_gpus=8), dict(ann_window='pre'), dict(num_matches=4),
               dict(num_matches=4, distinct_matches=True), dict(pq_m=16, pq_bits=6), dict(pq_m=8),
               dict(num_gpus=2, refine_k=512)):
        assert Config(index='ivfpq', pq_by_residual=False, **kw).pq_by_residual is False
    # an object that does not know the option (the reference's configuration) keeps the default
    assert Config.from_reference(dict(index='ivfpq')).pq_by_residual is True


def _hash_before_the_option(cfg):
    """``SpectralLibrary._get_index_hash`` as it was before ``pq_by_residual`` existed, restated."""
    hp = {k: cfg[k] for k in ('min_mz', 'max_mz', 'bin_size', 'hash_len', 'num_list')}
    if cfg.index == 'ivfflat' and cfg.kmeans_niter == 25 and cfg.seed == 1234 and cfg.flat_storage == 'fp32':
        return hashlib.sha1(json.dumps(hp).encode('utf-8')).hexdigest()
    d = dict(hp)
    d.update(index=cfg.index, kmeans_niter=cfg.kmeans_niter, seed=cfg.seed)
    if cfg.index == 'ivfflat' and cfg.flat_storage != 'fp32':
        d.update(flat_storage=cfg.flat_storage)
    if cfg.index == 'ivfpq':
        d.update(pq_m=cfg.pq_m, pq_bits=cfg.pq_bits)
        if cfg.refine_k:
            d.update(refine_k=cfg.refine_k)
    return hashlib.sha1(json.dumps(d).encode('utf-8')).hexdigest()


def test_index_hashes_move_only_when_the_mode_is_off():
    from ann_solo_amd.spectral_library import SpectralLibrary

    def hashes(cfg):
        sl = SpectralLibrary.__new__(SpectralLibrary)
        sl.config = cfg
        return sl._get_hyperparameter_hash(), sl._get_index_hash()
    existing = [dict(), dict(kmeans_niter=4), dict(seed=7), dict(flat_storage='fx22'), dict(num_list=4096),
                dict(index='ivfpq'), dict(index='ivfpq', pq_m=16, pq_bits=6), dict(index='ivfpq', refine_k=2048),
                dict(index='ivfpq', kmeans_niter=4, seed=4321, num_list=16), dict(index='ivfpq', ann_window='pre')]
    for kw in existing:
        for explicit in (dict(), dict(pq_by_residual=True)):
            cfg = Config.open_search(**kw, **explicit)
            assert hashes(cfg)[1] == _hash_before_the_option(cfg), kw
    seen = set()
    for kw in existing:
        if kw.get('index') != 'ivfpq':
            continue
        on, off = Config.open_search(**kw), Config.open_search(pq_by_residual=False, **kw)
        assert hashes(on)[0] == hashes(off)[0]                # the reference's own hash: untouched
        assert hashes(on)[1] != hashes(off)[1], kw
        seen.update((hashes(on)[1], hashes(off)[1]))
    assert len(seen) == 2 * sum(kw.get('index') == 'ivfpq' for kw in existing) - 2   # ann_window never hashes


def test_header_declares_and_library_exports_both_functions():
    from ann_solo_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'annsolo_mi.h')).read()
    assert re.search(r'int asl_index_set_by_residual\(asl_index_t \*idx, int32_t on\);', src)
    assert re.search(r'int asl_index_get_by_residual\(const asl_index_t \*idx\);', src)
    comment = src[:src.index('int asl_index_set_by_residual')].rsplit('/*', 1)[1]
    assert 'IndexIVFPQ::by_residual' in comment and 'dis0' in comment
    L = _lib.lib()
    for name in ('asl_index_set_by_residual', 'asl_index_get_by_residual'):
        assert hasattr(L, name) and name in _lib.EXPORTS
    # asl_index_info_t keeps its layout (ctypes mirrors depend on it)
    assert [f[0] for f in _lib.AslIndexInfo._fields_] == ['d', 'nlist', 'kind', 'pq_m', 'pq_ksub', 'pq_dsub', 'ntotal',
                                                          'nlocal', 'trained', 'shard_rank', 'shard_world']
    body = re.search(r'typedef struct\s*\{([^}]*)\}\s*asl_index_info_t;', src).group(1)
    assert 'by_residual' not in body


def test_null_handle_without_any_device_work():
    """Argument errors come before the device is touched: a null handle is ASL_ERR_INVALID (with or
    without a GPU), and the getter answers the default."""
    from ann_solo_amd import _lib
    L = _lib.lib()
    ASL_ERR_INVALID = int(re.search(r'#define ASL_ERR_INVALID \((-?\d+)\)',
                                    open(os.path.join(ROOT, 'include', 'annsolo_mi.h')).read()).group(1))
    assert L.asl_index_set_by_residual(None, 0) == ASL_ERR_INVALID
    assert b'null index' in L.asl_last_error()
    assert L.asl_index_get_by_residual(None) == 1
