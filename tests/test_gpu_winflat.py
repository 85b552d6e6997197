"""The window-exact index (`ASL_INDEX_WINFLAT`, `faiss_compat.IndexWindowFlat`, `Config.index = 'winflat'`): the k
best of ALL stored vectors whose key passes the query's precursor window, against tests/winflat_ref.py (numpy and
the oracle) -- ids exactly, scores as uint32 bits -- at the index level (block edges, ties and short rows, more
than FI_CHUNK blocks in a run, dense-row and all-zero queries, both storages) and through the fused hot path
(synchronous, pipelined, ranked, histograms, intervals, a search subset, ppm fragment tolerance)."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the native library loads: the process then holds one HIP runtime, torch's)

import winflat_ref as WR
from test_gpu_window_scan import _queries, _tie_library

pytestmark = pytest.mark.gpu

FI_BLK, FI_CHUNK = 832, 256            # csrc/flat_postings.hpp, csrc/flat_scan.hip
FIELDS = ('best_row', 'best_score', 'n_candidates', 'pm_count', 'pm_pairs')
STATE = 'error -3'                     # ASL_ERR_STATE in the message of AnnSoloMiError


def _sparse(n, d, nnz, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, d), np.float32)
    cols = rng.integers(0, d, (n, nnz))             # (a repeated column: fewer non-zeros)
    x[np.arange(n)[:, None], cols] = rng.random((n, nnz)).astype(np.float32) * 0.9 + 0.05
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _same_rows(D, I, rD, rI, tag):
    assert np.array_equal(I, rI), tag
    assert np.array_equal(np.asarray(D, np.float32).view(np.uint32), np.asarray(rD, np.float32).view(np.uint32)), tag


# ---------------------------------------------------------------------------------- 1, 4: block edges, query forms
N_EDGE = 2 * FI_BLK + 5


@pytest.fixture(scope='module')
def edge():
    rng = np.random.default_rng(11)
    xb = _sparse(N_EDGE, 800, 20, 12)
    rank = rng.permutation(N_EDGE)                  # rank[id]: the vector's position in key order
    key = (400.0 + 0.25 * rank).astype(np.float32)
    at = lambda r: 400.0 + 0.25 * r
    n = N_EDGE
    ranks = [(0, 0), (0, 1), (1, 1), (5, 831), (0, 831), (831, 832), (832, 832), (832, 833), (100, 200), (833, 1663),
             (832, 1663), (1663, 1664), (1664, n - 1), (n - 1, n - 1), (0, n - 1), (n - 1, n + 50), (-10, 3),
             (700, 1700)]
    W = [(at(a), at(b)) for a, b in ranks]
    W += [(400.05, 400.2), (500.0, 450.0), (np.nan, 500.0), (450.0, np.nan), (-np.inf, np.inf), (-np.inf, at(832)),
          (at(1663), np.inf), (at(n), np.inf)]
    W += [(at(0), at(n - 1)), (at(830), at(835)), (at(0), at(n - 1))]     # the dense-row, all-zero and 64-entry queries
    W = np.asarray(W, np.float64)
    xq = _sparse(len(W), 800, 24, 13)
    dense = np.zeros(800, np.float32)
    dense[rng.choice(800, 100, replace=False)] = rng.random(100).astype(np.float32) + 0.01    # > 64 non-zeros
    xq[-3] = dense
    xq[-2] = 0.0
    xq[-1] = 0.0
    xq[-1, rng.choice(800, 64, replace=False)] = rng.random(64).astype(np.float32) + 0.01     # exactly 64
    return xb, key, W, xq


@pytest.mark.parametrize('storage', ['fp32', 'fx22'])
def test_block_edges_and_query_forms(O, edge, storage):
    from ann_solo_amd import faiss_compat as faiss
    xb, key, W, xq = edge
    idx = faiss.IndexWindowFlat(800, storage=storage)
    assert idx.is_trained and idx.ntotal == 0 and idx.info().kind == 3
    idx.add(xb[:1000])
    idx.add(xb[1000:])
    assert idx.ntotal == N_EDGE
    stored = O.quantize_fx22(xb) if storage == 'fx22' else xb
    assert idx.flat_layout == (2 if storage == 'fx22' else 1)
    idx.set_window_key(key)
    keeps = [WR.mask(W[i], key, 0, 0.0, 'interval') for i in range(len(W))]
    sizes = [int(k.sum()) for k in keeps]
    assert 0 in sizes and 1 in sizes and N_EDGE in sizes and FI_BLK in sizes
    for k in (64, 1280):
        D, I = idx.search_window(xq, k, W, 0, 0.0, 'interval')
        rD, rI = WR.search(O, stored, xq, k, keeps)
        _same_rows(D, I, rD, rI, (storage, k))
        z = len(W) - 2                               # the all-zero query: score 0, the k lowest in-window ids
        ids = np.flatnonzero(keeps[z])[:k]
        assert np.array_equal(I[z][:len(ids)], ids) and (D[z][:len(ids)] == 0.0).all() and (I[z][len(ids):] == -1).all()
    # asl_index_search: the window that passes everything, in whatever order the layout has
    D, I = idx.search(xq, 64)
    rD, rI = O.flat_search(stored, xq, 64)
    _same_rows(D, I, rD, rI, (storage, 'search'))


# ---------------------------------------------------------------------------------- 2, 5, 9: the tie library
@pytest.fixture(scope='module')
def tie():
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib0, aux, lib = _tie_library()
    sl = SpectralLibrary(lib, config=Config.open_search(index='winflat', num_candidates=256))
    idx = sl._get_ann_index(2)
    xb = sl._encode(sl.partitions[2].spectra).cpu().numpy()
    yield lib0, aux, lib, sl, idx, xb
    sl.shutdown()


def test_ties_short_rows_and_scanned_count(O, tie):
    from ann_solo_amd import _lib
    lib0, aux, lib, sl, idx, xb = tie
    assert idx.info().kind == 3 and idx.ntotal == lib.n
    q = _queries(lib0, aux, 40, seed=72, with_copies=8)
    xq = sl._encode(q.to(sl.device)).cpu().numpy()
    q_pmz = q.numpy()[4].astype(np.float64)
    key0 = np.ascontiguousarray(sl.partitions[2].precursor_mz, np.float32)
    key_nan = key0.copy()
    key_nan[::7] = np.nan
    for i in range(0, 2000, 97):      # the vectorised window test is precursor_ok
        for tol, mode in ((300.0, 'Da'), (2e5, 'ppm')):
            assert bool(WR.mask(q_pmz[0], key0[i:i + 1], 2, tol, mode)[0]) == O.precursor_ok(q_pmz[0], key0[i], 2, tol, mode)
    cases = [(key0, 250.0, 'Da', 256), (key0, 250.0, 'Da', 1024), (key0, 2e5, 'ppm', 256), (key0, 2e5, 'ppm', 1024),
             (key0, 2.0, 'Da', 256), (key0, 2.0, 'Da', 1024), (key0, -1.0, 'Da', 256), (key0, -1.0, 'Da', 1024),
             (key0, 1e9, 'Da', 256), (key0, 1e9, 'Da', 1024), (key_nan, 300.0, 'Da', 256), (key_nan, 300.0, 'Da', 1024)]
    short_rows = 0
    L = _lib.lib()
    short_at = set()
    for key, tol, mode, k in cases:
        idx.set_window_key(key)
        keeps = [WR.mask(q_pmz[i], key, 2, tol, mode) for i in range(len(xq))]
        L.asl_profile_reset()
        L.asl_profile_enable(1)
        D, I = idx.search_window(xq, k, q_pmz, 2, tol, mode)
        L.asl_profile_enable(0)
        assert L.asl_profile_scanned_vectors() == sum(int(m.sum()) for m in keeps), (tol, mode)     # sum of hi - lo
        rD, rI = WR.search(O, xb, xq, k, keeps)
        _same_rows(D, I, rD, rI, (tol, mode, k))
        short_rows += int((I < 0).any(axis=1).sum())
        if 0 < tol < 1e9 and ((I < 0).any(axis=1) & (I[:, 0] >= 0)).any():
            short_at.add(k)               # a row that is neither empty nor full
        if tol < 0:
            assert (I == -1).all()
        if tol == 1e9:                # every finite key passes: asl_index_search itself
            D2, I2 = idx.search(xq, k)
            _same_rows(D, I, D2, I2, 'search')
    assert short_rows > 0 and short_at == {256, 1024}
    # ties at the k-th score: the copies of row 0 fill the rows of the first queries by ascending id
    idx.set_window_key(key0)
    keeps = [WR.mask(q_pmz[i], key0, 2, 250.0, 'Da') for i in range(8)]
    D, I = idx.search_window(xq[:8], 64, q_pmz[:8], 2, 250.0, 'Da')
    assert (I < 400).all() and (I >= 0).all()
    for i in range(8):
        assert np.array_equal(I[i], np.flatnonzero(keeps[i][:400])[:64]), i
    # equal keys straddling a block boundary: 700 vectors per key value, positions 700 .. 1399 cross 832
    key_eq = (400 + np.arange(lib.n) // 700).astype(np.float32)
    idx.set_window_key(key_eq)
    W = np.array([(401.0, 401.0), (400.0, 401.0), (401.0, 402.0), (400.5, 400.9), (406.0, 407.0), (401.0, 405.0)] * 2)
    keeps = [WR.mask(W[i], key_eq, 0, 0.0, 'interval') for i in range(len(W))]
    D, I = idx.search_window(xq[:len(W)], 256, W, 0, 0.0, 'interval')
    rD, rI = WR.search(O, xb, xq[:len(W)], 256, keeps)
    _same_rows(D, I, rD, rI, 'equal keys')


def _check_fused(O, sl, q, res, keeps, xb, key, k, rows=None):
    L = O.Spectra(*sl.partitions[2].spectra.to('cpu').numpy())
    for i in (range(q.n) if rows is None else rows):
        ref = WR.fused(O, q, i, L, xb, key, 2, keeps[i], k, res.pm_pairs.shape[1])
        assert np.array_equal(res.knn[i], ref['knn_I'][0]), i
        for f, g in (('n_candidates', 'n_cand'), ('best_row', 'best_row'), ('best_score', 'best_score'),
                     ('pm_count', 'pm_count')):
            assert getattr(res, f)[i] == ref[g][0], (f, i)
        n = res.pm_count[i]
        assert np.array_equal(res.pm_pairs[i, :n], ref['pm_pairs'][0, :n]), i


@pytest.mark.parametrize('tol,mode', [(250.0, 'Da'), (2e5, 'ppm'), (0.5, 'Da')])
def test_fused_path(O, tie, tol, mode):
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib0, aux, lib, _, _, xb = tie
    q = _queries(lib0, aux, 120, seed=73, with_copies=6)
    q_pmz = q.numpy()[4].astype(np.float64)
    cfg = Config.open_search(index='winflat', num_candidates=256, precursor_tolerance_mass_open=tol,
                             precursor_tolerance_mode_open=mode)
    sl = SpectralLibrary(lib, config=cfg)
    try:
        key = sl.partitions[2].precursor_mz
        keeps = [WR.mask(q_pmz[i], key, 2, tol, mode) for i in range(q.n)]
        res = sl._search_batch(q, 2, 'open', want_knn=True)
        _check_fused(O, sl, q, res, keeps, xb, key, 256)
        plain = sl._search_batch(q, 2, 'open')      # set-mode rows handed over with their lengths
        for f in FIELDS:
            assert np.array_equal(getattr(plain, f), getattr(res, f)), f
        sl.set_pipeline(True)
        try:
            qd = q.to('cuda:0')
            a_ = sl._search_batch(qd, 2, 'open', device_out=True)
            b_ = sl._search_batch(qd, 2, 'open', device_out=True, want_knn=True)
            sl.synchronize()
        finally:
            sl.set_pipeline(False)
        for r in (a_, b_):
            for f in FIELDS:
                got = getattr(r, f).cpu().numpy().astype(getattr(res, f).dtype)
                assert np.array_equal(got, getattr(res, f)), f
        assert np.array_equal(b_.knn.cpu().numpy(), res.knn)
        # ranked matches, their distinct form, the score histogram: rank 0 is the single-winner call
        sl.set_match_groups({2: (np.arange(lib.n) // 3).astype(np.int32)})
        for kw in (dict(), dict(distinct=True), dict(score_hist=True)):
            top = sl.search_batch_topn(q, 2, 'open', 5, want_knn=True, **kw)
            assert np.array_equal(top.knn, res.knn) and np.array_equal(top.n_candidates, res.n_candidates)
            for f in ('best_row', 'best_score', 'pm_count'):
                assert np.array_equal(getattr(top, f)[:, 0], getattr(res, f)), (f, kw)
            if 'score_hist' in kw:
                assert np.array_equal(top.score_hist.sum(axis=1), res.n_candidates)
    finally:
        sl.shutdown()


def test_fused_intervals_subset_and_the_candidate_lists(O, tie):
    lib0, aux, lib, sl, idx, xb = tie
    q = _queries(lib0, aux, 48, seed=74, with_copies=4)
    q_pmz = q.numpy()[4].astype(np.float64)
    key = sl.partitions[2].precursor_mz
    W = np.stack([q_pmz - 150.0, q_pmz + 500.0], 1)
    keeps = [WR.mask(W[i], key, 0, 0.0, 'interval') for i in range(q.n)]
    res = sl._search_batch(q, 2, 'open', want_knn=True, windows=W)
    _check_fused(O, sl, q, res, keeps, xb, key, 256)
    cands = sl._get_library_candidates(q, 2, 'open', windows=W)
    for i in range(q.n):
        assert np.array_equal(cands[i], np.sort(res.knn[i][res.knn[i] >= 0])), i
    with pytest.raises(ValueError):
        sl.candidate_rank(q, 2, np.zeros(q.n, np.int64))
    with pytest.raises(ValueError):
        sl.enable_sharding()
    # a search subset of about 10 %: the reference over the selected rows only
    tol, mode = sl._tolerance('open')
    sel = np.random.default_rng(9).random(lib.n) < 0.1
    sel[:400:3] = True
    sl.set_search_subset({2: sel})
    try:
        keeps = [WR.mask(q_pmz[i], key, 2, tol, mode) & sel for i in range(q.n)]
        sub = sl._search_batch(q, 2, 'open', want_knn=True)
        _check_fused(O, sl, q, sub, keeps, xb, key, 256)
        plain = sl._search_batch(q, 2, 'open')
        for f in FIELDS:
            assert np.array_equal(getattr(plain, f), getattr(sub, f)), f
    finally:
        sl.set_search_subset(None)
    keeps = [WR.mask(q_pmz[i], key, 2, tol, mode) for i in range(q.n)]
    _check_fused(O, sl, q, sl._search_batch(q, 2, 'open', want_knn=True), keeps, xb, key, 256, rows=range(0, q.n, 6))


def test_fused_ppm_fragment_tolerance(O, tie):
    import ppm_ref as PR
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib0, aux, lib, _, _, xb = tie
    q = _queries(lib0, aux, 6, seed=75, with_copies=2)
    q_pmz = q.numpy()[4].astype(np.float64)
    cfg = Config.open_search(index='winflat', num_candidates=64, precursor_tolerance_mass_open=100.0,
                             fragment_mz_tolerance=20.0, fragment_tolerance_unit='ppm')
    sl = SpectralLibrary(lib, config=cfg)
    try:
        key = sl.partitions[2].precursor_mz
        xq = sl._encode(q.to(sl.device)).cpu().numpy()
        keeps = [WR.mask(q_pmz[i], key, 2, 100.0, 'Da') for i in range(q.n)]
        _, rI = WR.search(O, xb, xq, 64, keeps)
        res = sl._search_batch(q, 2, 'open', want_knn=True)
        assert np.array_equal(res.knn, rI)
        Q, Lp = q.numpy(), sl.partitions[2].spectra.to('cpu').numpy()
        for i in range(q.n):
            rows = np.sort(rI[i][rI[i] >= 0])
            b, score, matches = PR.best_match(Q, i, Lp, rows, 20.0)
            assert res.best_row[i] == rows[b] and res.best_score[i] == score, i
            assert res.pm_count[i] == len(matches) and np.array_equal(res.pm_pairs[i, :len(matches)], matches), i
    finally:
        sl.shutdown()


# ---------------------------------------------------------------------------------- 3: chunk rollover
def test_more_blocks_than_a_chunk_in_one_run(O):
    """Runs of more than FI_CHUNK blocks: the unit table is refilled. 260 * 832 + 1 vectors -- 261 blocks, so that a
    run that starts in block 3 can still cover more than FI_CHUNK of them (256 * 832 + 1 vectors hold 257 blocks)."""
    from ann_solo_amd import faiss_compat as faiss
    n, d = 260 * FI_BLK + 1, 64
    xb = _sparse(n, d, 7, 21)
    idx = faiss.IndexWindowFlat(d)
    for a in range(0, n, 50000):
        idx.add(xb[a:a + 50000])
    assert idx.flat_layout == 1
    key = np.arange(n, dtype=np.float32)             # position = id
    idx.set_window_key(key)
    xq = _sparse(16, d, 7, 22)
    lo, hi = 3 * FI_BLK + 17, 259 * FI_BLK + 100
    assert hi // FI_BLK - lo // FI_BLK + 1 > FI_CHUNK
    W = np.array([(-np.inf, np.inf)] * 8 + [(float(lo), float(hi))] * 8)
    keeps = [WR.mask(W[i], key, 0, 0.0, 'interval') for i in range(16)]
    assert int(keeps[8].sum()) == hi - lo + 1
    D, I = idx.search_window(xq, 128, W, 0, 0.0, 'interval')
    rD, rI = WR.search(O, xb, xq, 128, keeps)
    _same_rows(D, I, rD, rI, 'rollover')


# ---------------------------------------------------------------------------------- 6: handle reuse
def test_key_follows_the_library_handle(O, tie):
    """One index searched with library A, then -- same handle -- with library B created after A was freed (same
    size, precursors +40 Da): the key must be B's."""
    from ann_solo_amd.packed import PackedSpectra
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib0, aux, libA, _, _, xb = tie
    o, mz, it, chg, pmz, pz = libA.numpy()
    libB = PackedSpectra.from_numpy(o, mz, it, chg, np.asarray(pmz, np.float64) + 40.0, pz)
    q = _queries(lib0, aux, 60, seed=77)
    q_pmz = q.numpy()[4].astype(np.float64)
    cfg = Config.open_search(index='winflat', num_candidates=256, precursor_tolerance_mass_open=60.0)
    slA = SpectralLibrary(libA, config=cfg)
    resA = slA._search_batch(q, 2, 'open', want_knn=True)
    idx = slA.partitions[2].index
    slA.partitions[2].index = None
    slA.shutdown()
    slB = SpectralLibrary(libB, config=cfg)
    try:
        slB.partitions[2].index = idx
        resB = slB._search_batch(q, 2, 'open', want_knn=True)
        assert not np.array_equal(resA.knn, resB.knn)
        key = slB.partitions[2].precursor_mz
        keeps = [WR.mask(q_pmz[i], key, 2, 60.0, 'Da') for i in range(q.n)]
        _check_fused(O, slB, q, resB, keeps, xb, key, 256)
    finally:
        slB.shutdown()


# ---------------------------------------------------------------------------------- 7, 8: lifetime, files, refusals
def test_layout_lifetime_files_and_refusals(O, tmp_path):
    from ann_solo_amd import _lib, faiss_compat as faiss
    from ann_solo_amd.spectral_library import Config
    L = _lib.lib()
    xb = _sparse(2000, 256, 9, 31)
    xq = _sparse(12, 256, 9, 32)
    key = np.random.default_rng(33).uniform(400, 1400, 2000).astype(np.float32)
    q_pmz = np.linspace(450.0, 1300.0, 12)
    idx = faiss.IndexWindowFlat(256)
    idx.add(xb[:1200])
    with pytest.raises(_lib.AnnSoloMiError, match=STATE):     # before a key is set
        idx.search_window(xq, 16, q_pmz, 2, 100.0)
    D, I = idx.search(xq, 16)                                 # needs no key
    _same_rows(D, I, *O.flat_search(xb[:1200], xq, 16), 'no key')
    assert L.asl_index_set_window_key(idx._h, 1199, _lib.ptr(key)) == -1      # ASL_ERR_INVALID: n != ntotal
    idx.set_window_key(key[:1200])
    keeps = [WR.mask(q_pmz[i], key[:1200], 2, 100.0, 'Da') for i in range(12)]
    _same_rows(*idx.search_window(xq, 16, q_pmz, 2, 100.0), *WR.search(O, xb[:1200], xq, 16, keeps), 'keyed')
    idx.add(xb[1200:])                                        # drops the layout and the key
    with pytest.raises(_lib.AnnSoloMiError, match=STATE):
        idx.search_window(xq, 16, q_pmz, 2, 100.0)
    with pytest.raises(_lib.AnnSoloMiError):
        idx.set_window_key(key[:1200])
    idx.set_window_key(key)
    keeps = [WR.mask(q_pmz[i], key, 2, 100.0, 'Da') for i in range(12)]
    want = WR.search(O, xb, xq, 16, keeps)
    got = idx.search_window(xq, 16, q_pmz, 2, 100.0)
    _same_rows(*got, *want, 'after add')
    # files: the kind and the vectors round-trip, the layout and the key do not
    path = str(tmp_path / 'w.idxmi')
    faiss.write_index(idx, path)
    back = faiss.read_index(path)
    info = back.info()
    assert (info.kind, info.d, info.ntotal, bool(info.trained)) == (3, 256, 2000, True) and back.storage == 'fp32'
    with pytest.raises(_lib.AnnSoloMiError, match=STATE):
        back.search_window(xq, 16, q_pmz, 2, 100.0)
    back.set_window_key(key)
    _same_rows(*back.search_window(xq, 16, q_pmz, 2, 100.0), *got, 'read_index')
    _same_rows(*back.search(xq, 16), *idx.search(xq, 16), 'read_index search')
    # an IVF-Flat file of this build against the bytes the parent commit wrote for the same data
    rng = np.random.default_rng(41)
    cen = _sparse(4, 32, 5, 42)
    x = _sparse(200, 32, 5, 43)
    lists = rng.integers(0, 4, 200).astype(np.int32)
    flat = faiss.IndexIVFFlat(faiss.IndexFlatIP(32), 32, 4)
    flat.set_trained(cen)
    _lib.check(L.asl_index_add_preassigned(flat._h, 200, _lib.ptr(x), _lib.ptr(lists)))
    p2 = str(tmp_path / 'f.idxmi')
    faiss.write_index(flat, p2)
    golden = os.path.join(os.path.dirname(__file__), 'golden', 'ivfflat_parent.idxmi')
    assert open(p2, 'rb').read() == open(golden, 'rb').read()
    # refusals: ASL_ERR_STATE with a reason, never a filter behind the top-k
    dev = torch.device('cuda', 0)
    dq = torch.from_numpy(xq).to(dev)
    dcD, dcI = torch.zeros((12, 1), device=dev), torch.zeros((12, 1), dtype=torch.int32, device=dev)
    dD, dI = torch.empty((12, 16), device=dev), torch.empty((12, 16), dtype=torch.int64, device=dev)
    dent = torch.zeros((12, 64, 2), dtype=torch.int32, device=dev)
    dcnt = torch.full((1,), 12, dtype=torch.int32, device=dev)
    comm = _lib.ptr(dcnt)                                     # any non-null pointer: the kind is refused before it is used
    for call in (lambda: idx.search_selected(xq, 16), lambda: idx.rank_of(xq, np.zeros(12, np.int64)),
                 lambda: idx.set_refine(64), lambda: idx.shard(0, 2), lambda: idx.shard_map(2),
                 lambda: idx.set_trained(cen), lambda: idx.search_window(xq, 1281, q_pmz, 2, 100.0),
                 lambda: idx.search(xq, 1281),
                 lambda: idx.search_preassigned(xq, 16, np.zeros((12, 1), np.float32), np.zeros((12, 1), np.int32)),
                 lambda: idx.search_preassigned_keys(xq, 16, np.zeros((12, 1), np.float32), np.zeros((12, 1), np.int32)),
                 lambda: _lib.check(L.asl_index_add_preassigned(idx._h, 12, _lib.ptr(xq), _lib.ptr(lists[:12]))),
                 lambda: _lib.check(L.asl_index_search_gated(idx._h, 12, _lib.ptr(dq), 16, 1, _lib.ptr(dcD), _lib.ptr(dcI),
                                                             _lib.ptr(dD), _lib.ptr(dI), _lib.ptr(dcnt))),
                 lambda: _lib.check(L.asl_index_search_entries(idx._h, 12, _lib.ptr(dent), _lib.ptr(dcI), 16, 1,
                                                               _lib.ptr(dcD), _lib.ptr(dcI), _lib.ptr(dD), _lib.ptr(dI),
                                                               None)),
                 lambda: idx.search_entries_keys(dent, dcI[:, 0].contiguous(), 16, dcD, dcI),
                 lambda: _lib.check(L.asl_index_search_sharded(idx._h, comm, 12, _lib.ptr(dq), 16, 1, _lib.ptr(dD),
                                                               _lib.ptr(dI))),
                 lambda: _lib.check(L.asl_index_search_sharded_ex(idx._h, comm, 12, _lib.ptr(dq), 16, 1, _lib.ptr(dD),
                                                                  _lib.ptr(dI), 0, 0, -1)),
                 lambda: _lib.check(L.asl_index_set_by_residual(idx._h, 0))):
        with pytest.raises(_lib.AnnSoloMiError, match=STATE):
            call()
    idx.set_unordered(2)                                      # packed-key rows
    try:
        with pytest.raises(_lib.AnnSoloMiError, match=STATE):
            idx.search(xq, 16)
    finally:
        idx.set_unordered(0)
    assert L.asl_index_set_window_scan(idx._h, 1) == 0 and L.asl_index_set_window_scan(idx._h, 0) == 0     # no-ops
    dense = faiss.IndexWindowFlat(32)                         # too dense for postings: 5 * 8 >= 32
    dense.add(x)
    with pytest.raises(_lib.AnnSoloMiError, match=STATE + '.*sparse'):
        dense.search(x[:4], 8)
    zeros = faiss.IndexWindowFlat(32)                         # nothing to build postings from
    zeros.add(np.zeros((40, 32), np.float32))
    with pytest.raises(_lib.AnnSoloMiError, match=STATE + '.*all-zero'):
        zeros.search(x[:4], 8)
    _same_rows(*got, *idx.search_window(xq, 16, q_pmz, 2, 100.0), 'after the refusals')
    for bad in (dict(num_gpus=2), dict(refine_k=512), dict(ann_window='pre'), dict(pq_by_residual=False)):
        with pytest.raises(ValueError):
            Config.open_search(index='winflat', **bad)
