"""The look-up address of the tiled IVF-PQ scan as one v_dot4_u32_u8 (csrc/pq_tile.hpp, lut_at2), in the
instantiations that test_gpu_pq_adc_address.py does not reach: every code byte value at every one of the 32 byte
positions, ids and score bits against the oracle (O.HostIVF.search), no tolerance.

That file runs the 2048-key kernels at k = 64 and 512. The address is byte * 128 + the lane's LDS address of its table
column, and what differs between the instantiations is the lane's part:

  * the 4096-key kernels (k = 1281, the smallest k that leaves the 2048-key kernel, and k = 2048) keep the table behind
    a 32 KB key buffer, so the addresses pass 2^16: a form that keeps 16 address bits fails here and nowhere else;
  * two probes per thread (nprobe = 513, the smallest that selects it) with either key buffer, on an index of 520
    lists: the long designed list, the lists of 1 / 63 / 64 / 65 vectors, and 515 lists of one vector each;
  * the selected scan with every other vector selected, the window scan with windows that cut the long list's run
    inside a tile (the first lane non-zero, the end lane below 63);
  * a set-mode search with the scan-side post-filter through the batch entry of the benchmark, at 64 queries (there the
    codes are the trained quantiser's, not designed);
  * rank_of (rank_scan.hip, tile_adc<0>) against the rows of k = 1281.

The codes are made by hand as there: 256 pairwise distinct dyadic codewords per sub-quantiser, a vector is its list's
centroid plus chosen codewords, so the residual is the codeword exactly and the encoder must return the chosen code.
Row i < 256 of the long list has c_m = (i + 37 m) mod 256 (every byte value at every position); then rows of all-0,
all-255, all-127 and all-128. Queries: every table column live and distinct, one live column, all zero, hashed spectra.
Both code layouts (set_scan_variant 0 and 2) wherever the instantiation has both."""
import ctypes as C

import numpy as np
import pytest

import interval_ref as IR
import selector_ref as SR

D, M = 800, 32
DSUB = D // M
SIZES = [256 + 4, 1, 63, 64, 65]
NLIST_S, NLIST_W = 5, 520                     # the small index, and the one for two probes per thread
NPROBE_W = 513
NQ = 8
Q_ALL_LIVE, Q_ONE_LIVE, Q_ZERO = 0, 1, 2
KS_S = (64, 1281, 2048)
KS_W = (512, 1281)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _design(nlist, seed):
    """(vectors, lists, codes, centroids, codebooks): SIZES in the first five lists, one vector in every other."""
    rng = np.random.default_rng(seed)
    cb = (rng.integers(-32, 33, size=(M, 256, DSUB)) / 64.0).astype(np.float32)
    for m in range(M):
        assert len(np.unique(cb[m], axis=0)) == 256            # pairwise distinct codewords
    cen = (rng.integers(-32, 33, size=(nlist, D)) / 64.0).astype(np.float32)
    sizes = SIZES + [1] * (nlist - len(SIZES))
    n = sum(sizes)
    m = np.arange(M)
    codes = np.empty((n, M), np.int64)
    i = np.arange(256)
    codes[:256] = (i[:, None] + 37 * m[None, :]) % 256
    codes[256], codes[257], codes[258], codes[259] = 0, 255, 127, 128
    r = np.arange(n - 260)
    codes[260:] = (5 * r[:, None] + 91 * m[None, :] + 3) % 256
    codes = codes.astype(np.uint8)
    assign = np.repeat(np.arange(nlist, dtype=np.int32), sizes)
    x = cen[assign].copy()
    for mm in range(M):
        x[:, mm * DSUB:(mm + 1) * DSUB] += cb[mm, codes[:, mm]]   # exact: multiples of 1/64 below 2
    for mm in range(M):
        assert len(np.unique(codes[:256, mm])) == 256
    perm = rng.permutation(n)                                  # rows in an order that is not the lists'
    return x[perm], assign[perm], codes[perm], cen, cb


def _queries(O):
    from ann_solo_amd import synthetic
    lib, aux = synthetic.make_library(64, seed=311, device='cpu')
    q, _ = synthetic.make_queries(lib, aux, NQ, seed=312)
    o, mz, inten, *_ = q.numpy()
    xq = O.encode_batch(mz, inten, o, 10.96, 0.04, D)
    rng = np.random.default_rng(99)
    xq[Q_ALL_LIVE] = 0.0
    dims = np.array([m * DSUB + (m * 7) % DSUB for m in range(M)])
    xq[Q_ALL_LIVE, dims] = (rng.permutation(M) + 1).astype(np.float32) / np.float32(64.0)
    xq[Q_ONE_LIVE] = 0.0
    xq[Q_ONE_LIVE, 21 * DSUB + np.array([0, 11, 24])] = np.array([0.5, 0.25, 0.75], np.float32)
    xq[Q_ZERO] = 0.0
    live = np.array([len(np.unique(np.nonzero(r)[0] // DSUB)) for r in xq])
    assert live[Q_ALL_LIVE] == M and live[Q_ONE_LIVE] == 1 and live[Q_ZERO] == 0
    assert (live[Q_ZERO + 1:] > 1).all()
    return xq


def _world(O, nlist, seed):
    x, assign, codes, cen, cb = _design(nlist, seed)
    # the design check, on the CPU: the oracle's encoder returns exactly the designed codes
    assert np.array_equal(O.pq_encode(x, cen, assign, cb), codes)
    return dict(x=x, assign=assign, codes=codes, cen=cen, cb=cb, ivf=O.HostIVF(cen, assign, codes, cb),
                xq=_queries(O), nlist=nlist, rows={})


def _rows(w, k, nprobe):
    """The oracle's answer, computed once per (k, nprobe) and shared."""
    if (k, nprobe) not in w['rows']:
        w['rows'][k, nprobe] = w['ivf'].search(w['xq'], k, nprobe)
    return w['rows'][k, nprobe]


@pytest.fixture(scope='module')
def small(O):
    return _world(O, NLIST_S, 20817)


@pytest.fixture(scope='module')
def wide(O):
    return _world(O, NLIST_W, 20818)


def _index(w):
    from ann_solo_amd import _lib
    from ann_solo_amd import faiss_compat as faiss
    idx = faiss.IndexIVFPQ(faiss.IndexFlatIP(D), D, w['nlist'], M, 8)
    idx.set_trained(w['cen'], w['cb'])
    x = np.ascontiguousarray(w['x'], np.float32)
    lists = np.ascontiguousarray(w['assign'], np.int32)
    _lib.check(_lib.lib().asl_index_add_preassigned(idx._h, C.c_int64(len(x)), x.ctypes.data_as(C.c_void_p),
                                                    lists.ctypes.data_as(C.c_void_p)))
    return idx


@pytest.fixture(scope='module')
def small_index(small):
    return _index(small)


@pytest.fixture(scope='module')
def wide_index(wide):
    return _index(wide)


@pytest.mark.parametrize('which', ['small', 'wide'])
def test_the_oracle_encodes_the_designed_codes(O, small, wide, which):
    w = small if which == 'small' else wide                    # (the fixtures assert pq_encode == the design)
    codes, assign = w['codes'], w['assign']
    long_list = codes[assign == 0]
    assert len(long_list) == 260
    for m in range(M):
        assert len(np.unique(long_list[:, m])) == 256          # every byte value at every position
    for v in (0, 255, 127, 128):
        assert (long_list == v).all(1).any()
    sizes = SIZES + [1] * (w['nlist'] - len(SIZES))
    assert np.array_equal(np.diff(w['ivf'].list_offsets), sizes)
    lut = O.pq_lut(w['xq'][Q_ALL_LIVE], w['cb'])
    assert (lut != 0).any(1).all() and len(np.unique(lut, axis=0)) == M
    assert (O.pq_lut(w['xq'][Q_ONE_LIVE], w['cb']) != 0).any(1).sum() == 1


def _assert_equal(got, want):
    (Dg, Ig), (Do, Io) = got, want
    assert np.array_equal(Ig, Io), np.nonzero((Ig != Io).any(1))[0]
    assert np.array_equal(_bits(Dg), _bits(Do)), np.nonzero((_bits(Dg) != _bits(Do)).any(1))[0]


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['small', 'wide'])
def test_the_index_holds_the_designed_codes(small, wide, small_index, wide_index, which):
    w, idx = (small, small_index) if which == 'small' else (wide, wide_index)
    off, ids, codes = idx.lists()
    assert np.array_equal(off, w['ivf'].list_offsets) and np.array_equal(ids, w['ivf'].ids)
    assert np.array_equal(codes, w['codes'][ids])


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [0, 2])
@pytest.mark.parametrize('k', KS_S)
def test_the_4096_key_kernels_equal_the_oracle(small, small_index, k, variant):
    """k = 1281 and 2048: the table behind the 32 KB key buffer (k = 64: the same index on the 2048-key kernel)."""
    small_index.nprobe = NLIST_S
    small_index.set_scan_variant(variant)
    got = small_index.search(small['xq'], k)
    assert small_index.codes_mmajor or variant == 2
    want = _rows(small, k, NLIST_S)
    assert ((want[1] >= 0).sum(1) == min(k, sum(SIZES))).all()
    _assert_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [0, 2])
@pytest.mark.parametrize('k', KS_W)
def test_two_probes_per_thread_equal_the_oracle(wide, wide_index, k, variant):
    wide_index.nprobe = NPROBE_W
    wide_index.set_scan_variant(variant)
    got = wide_index.search(wide['xq'], k)
    assert wide_index.codes_mmajor or variant == 2
    want = _rows(wide, k, NPROBE_W)
    assert (want[1][:, 0] >= 0).all()
    _assert_equal(got, want)


@pytest.mark.gpu
def test_the_selected_scan_equals_the_oracle(O, small, small_index):
    keep = np.arange(len(small['x'])) % 2 == 0                 # every other vector
    small_index.nprobe = NLIST_S
    small_index.set_scan_variant(0)
    small_index.set_selector(keep)
    try:
        got = small_index.search_selected(small['xq'], 64)
        SR.assert_rows_equal(got, SR.search_selected(O, small['ivf'], small['xq'], 64, NLIST_S, keep))
        hit = got[1][got[1] >= 0]
        assert keep[hit].all() and len(hit) == 64 * NQ
    finally:
        small_index.set_selector(None)


@pytest.mark.gpu
def test_the_window_scan_cut_inside_a_tile_equals_the_oracle(O, small, small_index):
    """A vector's key is 500 + its rank in its list, so the window [a, b] of ranks is the run [a, b] of the
    window-ordered list: of the long list's five tiles (260 vectors) it starts at lane a mod 64 and ends at b mod 64."""
    ivf = small['ivf']
    key = np.empty(len(small['x']), np.float32)
    for l in range(NLIST_S):
        ids = ivf.ids[ivf.list_offsets[l]:ivf.list_offsets[l + 1]]
        key[ids] = 500.0 + np.arange(len(ids), dtype=np.float32)
    windows = ((5, 200), (70, 130), (1, 62), (129, 258))
    for a, b in windows:
        assert a % 64 != 0 and b % 64 < 63
    wins = np.array([[500.0 + windows[i % 4][0] - 0.25, 500.0 + windows[i % 4][1] + 0.25] for i in range(NQ)])
    small_index.nprobe = NLIST_S
    small_index.set_scan_variant(0)
    small_index.set_window_key(key)
    for k in (64, 512):
        got = small_index.search_window(small['xq'], k, wins, 2, 0.0, 'interval')
        IR.assert_rows_equal(got, IR.index_rows(O, ivf, small['xq'], k, NLIST_S, key, wins))
        assert (got[1][:, 0] >= 0).all()


@pytest.mark.gpu
def test_rank_of_agrees_with_the_rows_of_k_1281(small, small_index):
    n = sum(SIZES)
    Do, Io = _rows(small, 1281, NLIST_S)
    small_index.nprobe = NLIST_S
    for shift in (0, 131, 259, 260, 452):
        T = ((np.arange(NQ) * 57 + shift) % n).astype(np.int64)
        rank, score, scope = small_index.rank_of(small['xq'], T, 0)
        want = np.array([int(np.nonzero(Io[i] == T[i])[0][0]) for i in range(NQ)])
        assert np.array_equal(rank, want), (shift, rank, want)
        assert (scope == n).all()
        assert np.array_equal(_bits(score), _bits(Do[np.arange(NQ), want]))


@pytest.mark.gpu
def test_set_mode_batch_with_the_scan_side_post_filter(O):
    """The batch entry of the benchmark (set-mode rows, the precursor filter in the scan's finish), 64 queries:
    winners, scores and candidate counts against the oracle's batch, both code layouts."""
    from ann_solo_amd import _lib, synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, aux = synthetic.make_library(2500, seed=913, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, 64, seed=914, charge=2)
    cfg = Config.open_search(num_list=8, num_probe=8, num_candidates=64, index='ivfpq', kmeans_niter=3,
                             precursor_tolerance_mass_open=500, precursor_tolerance_mode_open='Da')
    prev = _lib.lib().asl_set_scan_postfilter(1)
    sl = SpectralLibrary(lib, config=cfg, device='cuda:0')
    try:
        part = sl.partitions[2]
        idx = sl._get_ann_index(2)
        ivf = SR.host_ivf(O, idx)
        first = sl._search_batch(q, 2, 'open')
        ref = O.search_batch(O.Spectra(*q.numpy()), O.Spectra(*part.spectra.to('cpu').numpy()), part.precursor_mz,
                             2, ivf, 64, 8, 500, 'Da', 0.02, True, pm_stride=first.pm_pairs.shape[1])
        assert (ref['best_row'] >= 0).mean() > 0.5
        for variant in (2, 0):
            idx.set_scan_variant(variant)
            r = sl._search_batch(q, 2, 'open')
            assert np.array_equal(r.best_row, ref['best_row']), variant
            assert np.array_equal(r.best_score, ref['best_score']), variant
            assert np.array_equal(r.n_candidates, ref['n_cand']), variant
            assert np.array_equal(r.pm_count, ref['pm_count']), variant
    finally:
        sl.shutdown()
        _lib.lib().asl_set_scan_postfilter(prev)
