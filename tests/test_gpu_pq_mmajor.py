"""The tiled IVF-PQ scan over the sub-quantiser-major copy of the codes (asl_index_set_scan_variant 0, the
default) against the same scan over the tile-major codes (variant 2) in the same process, and both against
the oracle: ids and score bits equal, no tolerance. The new path loads a tile's code bytes only in the lanes
whose sub-quantiser has a non-zero query component; everything behind the loads is shared, so what can go
wrong is the copy (a list's last tile, the plane padding, an empty list), the live mask (no, one, all
sub-vectors live; the dense-row fallback above 64 non-zeros) and a stale copy after add().

The index: d = 800, m = 32, 8 bits, 64 lists filled through asl_index_add_preassigned, so that the list
sizes are what the generator says: an empty list, lists of 1, 7, 16, 63, 64, 65, 128 and 129 vectors (one,
two and three tiles), one list of 3 000 copies of ONE vector (equal scores beyond the 2 048-key buffer:
refused reservations and the exact flushes), the rest between 300 and 419 (five to seven tiles)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, M, NLIST, NITER, SEED = 800, 32, 64, 2, 9731
DSUB = D // M
SPECIAL = {0: 0, 1: 7, 2: 64, 3: 65, 4: 128, 5: 129, 6: 1, 7: 16, 8: 63}
DUP_LIST, DUP_N = 9, 3000
NQ = 256
# query rows made by hand (the others are hashed spectra, about 33 non-zeros as the benchmark's)
Q_ZERO, Q_ALL_LIVE, Q_ONE_LIVE, Q_DENSE, Q_64, Q_65, Q_DUP = 0, 1, 2, 3, 4, 5, 6


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _sizes():
    s = [SPECIAL.get(l, 300 + (l * 13) % 120) for l in range(NLIST)]
    s[DUP_LIST] = DUP_N
    return np.array(s, np.int64)


def _sparse_row(rng, dims):
    x = np.zeros(D, np.float32)
    x[dims] = rng.random(len(dims)).astype(np.float32) + 0.1
    return x / np.float32(np.sqrt((x.astype(np.float64) ** 2).sum()))


@pytest.fixture(scope='module')
def world(O):
    """Vectors, their lists, the oracle's quantisers, codes and inverted lists; the queries; the oracle's answers
    by (k, nprobe), computed once."""
    from ann_solo_amd import synthetic
    sizes = _sizes()
    n = int(sizes.sum())
    assert 19000 <= n <= 24000
    lib, aux = synthetic.make_library(n, seed=171, device='cpu')
    q, _ = synthetic.make_queries(lib, aux, NQ, seed=172)
    o, mz, inten, *_ = lib.numpy()
    xb = O.encode_batch(mz, inten, o, 10.96, 0.04, D)
    o, mz, inten, *_ = q.numpy()
    xq = O.encode_batch(mz, inten, o, 10.96, 0.04, D)
    rng = np.random.default_rng(SEED)
    assign = rng.permutation(np.repeat(np.arange(NLIST, dtype=np.int32), sizes))
    dup_rows = np.nonzero(assign == DUP_LIST)[0]
    xb[dup_rows] = xb[dup_rows[0]]
    cen = O.kmeans(xb[:4000], NLIST, NITER, SEED, 0, 256)
    cb = O.pq_train(xb[:4000], cen, M, 256, NITER, SEED + 7)
    codes = O.pq_encode(xb, cen, assign, cb)
    ivf = O.HostIVF(cen, assign, codes, cb)
    # the hand-made rows
    xq[Q_ZERO] = 0.0
    xq[Q_ALL_LIVE] = _sparse_row(rng, np.array([m * DSUB + (m * 7) % DSUB for m in range(M)]))
    xq[Q_ONE_LIVE] = _sparse_row(rng, 17 * DSUB + np.array([0, 11, 24]))
    xq[Q_DENSE] = _sparse_row(rng, np.sort(rng.choice(D, 100, replace=False)))
    xq[Q_64] = _sparse_row(rng, np.sort(rng.choice(D, 64, replace=False)))
    xq[Q_65] = _sparse_row(rng, np.sort(rng.choice(D, 65, replace=False)))
    xq[Q_DUP] = xb[dup_rows[0]]
    nnz = (xq != 0).sum(1)
    live = np.array([len(np.unique(np.nonzero(r)[0] // DSUB)) for r in xq])
    assert nnz[Q_ZERO] == 0 and live[Q_ALL_LIVE] == M and live[Q_ONE_LIVE] == 1
    assert nnz[Q_DENSE] == 100 and nnz[Q_64] == 64 and nnz[Q_65] == 65
    rest = np.arange(NQ) > Q_DUP
    assert 25 <= nnz[rest].mean() <= 45 and nnz[rest].max() <= 64        # bench-like rows: the entry-list path
    assert 0.4 <= live[rest].mean() / M <= 0.8                            # ... with dead sub-quantisers in them
    answers = {}

    def oracle(k, nprobe):
        if (k, nprobe) not in answers:
            answers[(k, nprobe)] = ivf.search(xq, k, nprobe)
        return answers[(k, nprobe)]
    return dict(xb=xb, xq=xq, assign=assign, cen=cen, cb=cb, ivf=ivf, sizes=sizes, oracle=oracle)


def _add(idx, x, lists):
    from ann_solo_amd import _lib
    x = np.ascontiguousarray(x, np.float32)
    lists = np.ascontiguousarray(lists, np.int32)
    _lib.check(_lib.lib().asl_index_add_preassigned(idx._h, C.c_int64(len(x)), x.ctypes.data_as(C.c_void_p),
                                                    lists.ctypes.data_as(C.c_void_p)))


def _new_index(w, upto=None):
    from ann_solo_amd import faiss_compat as faiss
    idx = faiss.IndexIVFPQ(faiss.IndexFlatIP(D), D, NLIST, M, 8)
    idx.set_trained(w['cen'], w['cb'])
    _add(idx, w['xb'][:upto], w['assign'][:upto])
    return idx


@pytest.fixture(scope='module')
def index(world):
    return _new_index(world)


def test_the_lists_hold_every_edge_the_copy_has(world, index):
    off, ids, codes = index.lists()
    ivf = world['ivf']
    assert np.array_equal(off, ivf.list_offsets) and np.array_equal(ids, ivf.ids)
    assert np.array_equal(codes, ivf.payload)
    size = np.diff(off)
    assert np.array_equal(size, world['sizes'])
    tiles = (size + 63) // 64
    assert (size == 0).any() and ((size > 0) & (size < 16)).any()
    assert (size == 64).any() and (size == 65).any() and (size == 63).any() and (size == 16).any()
    assert (tiles[size > 0] % 2 == 1).any() and (tiles[size > 0] % 2 == 0).any()
    assert size[DUP_LIST] == DUP_N > 2048


@pytest.mark.parametrize('nprobe', [1, 8, NLIST])
@pytest.mark.parametrize('k', [1, 100, 1024])
def test_both_code_layouts_and_the_oracle_agree(world, index, k, nprobe):
    xq = world['xq']
    index.nprobe = nprobe
    index.set_scan_variant(2)
    Dt, It = index.search(xq, k)
    index.set_scan_variant(0)
    Dm, Im = index.search(xq, k)
    assert index.codes_mmajor                      # the default path did scan the sub-quantiser-major copy
    Do, Io = world['oracle'](k, nprobe)
    assert np.array_equal(Im, It) and np.array_equal(_bits(Dm), _bits(Dt))
    assert np.array_equal(Im, Io) and np.array_equal(_bits(Dm), _bits(Do))
    if k == 1024 and nprobe == NLIST:
        # the tie cases are in the rows compared: the all-zero query scores every vector alike, and the 3 000
        # copies of one vector are one block of equal scores, larger than the key buffer, that k cuts through
        assert (Do[Q_ZERO] == Do[Q_ZERO, 0]).all() and (np.diff(Io[Q_ZERO]) > 0).all()
        dup = np.isin(Io[Q_DUP], np.nonzero(world['assign'] == DUP_LIST)[0])
        assert dup[-1] and dup.sum() > 900 and len(np.unique(Do[Q_DUP][dup])) == 1
        assert (np.diff(Io[Q_DUP][dup]) > 0).all()


def test_variant_2_never_builds_the_copy(world):
    idx = _new_index(world, 3000)
    idx.set_scan_variant(2)
    idx.nprobe = 8
    D2, I2 = idx.search(world['xq'], 100)
    assert not idx.codes_mmajor
    idx.set_scan_variant(0)
    D0, I0 = idx.search(world['xq'], 100)
    assert idx.codes_mmajor
    assert np.array_equal(I0, I2) and np.array_equal(_bits(D0), _bits(D2))


def test_add_after_a_search_rebuilds_the_copy(world, index):
    n = len(world['xb'])
    idx = _new_index(world, n // 2)
    idx.nprobe = 8
    idx.search(world['xq'], 100)
    assert idx.codes_mmajor
    _add(idx, world['xb'][n // 2:], world['assign'][n // 2:])
    assert not idx.codes_mmajor                    # the lists changed: the copy is stale until the next search
    D, I = idx.search(world['xq'], 100)
    assert idx.codes_mmajor
    index.nprobe = 8
    index.set_scan_variant(0)
    Df, If = index.search(world['xq'], 100)        # the index that was filled in one go
    Do, Io = world['oracle'](100, 8)
    assert np.array_equal(I, If) and np.array_equal(_bits(D), _bits(Df))
    assert np.array_equal(I, Io) and np.array_equal(_bits(D), _bits(Do))


def test_set_mode_with_the_post_filter_as_the_batch_search_uses_it(O):
    """asl_search_batch's scan: unordered int32 rows, the precursor post-filter in the scan's finish. Winners,
    scores, candidate counts and peak matches under both code layouts equal the oracle's."""
    from ann_solo_amd import synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, aux = synthetic.make_library(3000, seed=181, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, 96, seed=182, charge=2)
    cfg = Config.open_search(num_list=16, num_probe=6, num_candidates=128, index='ivfpq', kmeans_niter=3,
                             precursor_tolerance_mass_open=500, precursor_tolerance_mode_open='Da')
    sl = SpectralLibrary(lib, config=cfg, device='cuda:0')
    try:
        part = sl.partitions[2]
        idx = sl._get_ann_index(2)
        info = idx.info()
        assert (info.pq_m, info.pq_ksub) == (32, 256)
        off, ids, codes = idx.lists()
        ivf = O.HostIVF.__new__(O.HostIVF)
        ivf.centroids, ivf.nlist, ivf.d = idx.centroids(), info.nlist, info.d
        ivf.list_offsets, ivf.ids, ivf.payload, ivf.codebooks, ivf.kind = off, ids, codes, idx.codebooks(), 1
        idx.set_scan_variant(2)
        first = sl._search_batch(q, 2, 'open')
        assert not idx.codes_mmajor                # nothing asked for the copy so far
        ref = O.search_batch(O.Spectra(*q.numpy()), O.Spectra(*part.spectra.to('cpu').numpy()), part.precursor_mz,
                             2, ivf, 128, 6, 500, 'Da', 0.02, True, pm_stride=first.pm_pairs.shape[1])
        assert (ref['best_row'] >= 0).mean() > 0.5
        for variant in (2, 0, 2, 0):
            idx.set_scan_variant(variant)
            r = sl._search_batch(q, 2, 'open')
            if variant == 0:
                assert idx.codes_mmajor            # built by the first default batch, then kept
            assert np.array_equal(r.best_row, ref['best_row']), variant
            assert np.array_equal(r.best_score, ref['best_score']), variant
            assert np.array_equal(r.n_candidates, ref['n_cand']), variant
            assert np.array_equal(r.pm_count, ref['pm_count']), variant
        assert idx.codes_mmajor
    finally:
        sl.shutdown()
