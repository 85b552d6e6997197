"""The window scan (`Config.ann_window = 'pre'`, asl_index_search_window / asl_index_set_window_scan):
the k best vectors of the probed lists AMONG those that pass the query's precursor window, against the
oracle's IVF-PQ search over lists that keep only that query's in-window vectors (same centroids, same
codebooks, same codes) -- identical ids, identical score bits, and through the fused hot path identical
winners, scores, candidate counts and peak matches, synchronous and pipelined."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ('best_row', 'best_score', 'n_candidates', 'pm_count', 'pm_pairs')


def _window_mask(q_pmz, key, charge, tol, mode):
    """precursor_ok (csrc/common.hpp) over a key column, in the same double arithmetic."""
    l = np.asarray(key, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        if mode == 'Da':
            return np.abs(q_pmz - l) * float(charge) <= tol
        return np.abs(q_pmz - l) / l * 1000000.0 <= tol


def _host_ivf(O, idx):
    off, ids, payload = idx.lists()
    info = idx.info()
    ivf = O.HostIVF.__new__(O.HostIVF)
    ivf.centroids, ivf.nlist, ivf.d = idx.centroids(), info.nlist, info.d
    ivf.list_offsets, ivf.ids, ivf.payload, ivf.codebooks = off, ids, payload, idx.codebooks()
    ivf.kind = 1
    return ivf


def _filtered(O, ivf, keep_by_id):
    """The oracle's IVF with only the vectors whose id is kept (same lists, same order inside a list)."""
    keep = keep_by_id[ivf.ids]
    lst = np.repeat(np.arange(ivf.nlist), np.diff(ivf.list_offsets))
    out = O.HostIVF.__new__(O.HostIVF)
    out.centroids, out.nlist, out.d, out.codebooks, out.kind = ivf.centroids, ivf.nlist, ivf.d, ivf.codebooks, 1
    out.list_offsets = np.concatenate([[0], np.cumsum(np.bincount(lst[keep], minlength=ivf.nlist))]).astype(np.int32)
    out.ids = np.ascontiguousarray(ivf.ids[keep])
    out.payload = np.ascontiguousarray(ivf.payload[keep])
    return out


def _tie_library(n=5000, seed=71):
    """synthetic library whose rows 0 .. 399 are copies of row 0 spread over +-300 Da (score ties)."""
    from ann_solo_amd import synthetic
    from ann_solo_amd.packed import PackedSpectra
    lib0, aux = synthetic.make_library(n, seed=seed, device='cpu', charges=(2,), charge_p=(1.0,))
    o, mz, it, chg, pmz, pz = lib0.numpy()
    a, b = int(o[0]), int(o[1])
    rng = np.random.default_rng(5)
    offs = [0]
    MZ, IT, CH, PM = [], [], [], []
    for r in range(lib0.n):
        s, e = (a, b) if r < 400 else (int(o[r]), int(o[r + 1]))
        MZ.append(mz[s:e]); IT.append(it[s:e]); CH.append(chg[s:e])
        PM.append(pmz[0] + rng.uniform(-300, 300) if r < 400 else pmz[r])
        offs.append(offs[-1] + (e - s))
    lib = PackedSpectra.from_numpy(np.asarray(offs, np.int32), np.concatenate(MZ), np.concatenate(IT),
                                   np.concatenate(CH), np.asarray(PM), pz)
    return lib0, aux, lib


def _queries(lib0, aux, nq, seed, with_copies=0):
    """queries of make_queries; the first `with_copies` become row 0's spectrum (the tie block's)."""
    from ann_solo_amd import synthetic
    from ann_solo_amd.packed import PackedSpectra
    q, _ = synthetic.make_queries(lib0, aux, nq, seed=seed, charge=2)
    qo, qmz, qit, qchg, qpmz, qpz = q.numpy()
    o, mz, it, chg, pmz, pz = lib0.numpy()
    a, b = int(o[0]), int(o[1])
    offs, MZ, IT, CH = [0], [], [], []
    for i in range(q.n):
        s, e = int(qo[i]), int(qo[i + 1])
        src = (mz[a:b], it[a:b], chg[a:b]) if i < with_copies else (qmz[s:e], qit[s:e], qchg[s:e])
        MZ.append(src[0]); IT.append(src[1]); CH.append(src[2])
        offs.append(offs[-1] + len(src[0]))
    qp = np.array(qpmz, np.float64)
    qp[:with_copies] = pmz[0] + 7.0
    return PackedSpectra.from_numpy(np.asarray(offs, np.int32), np.concatenate(MZ), np.concatenate(IT),
                                    np.concatenate(CH), qp, qpz)


def _spectra_rows(O, q, rows):
    o, mz, it, chg, pmz, pz = q.numpy()
    sel = [(int(o[i]), int(o[i + 1])) for i in rows]
    offs = np.concatenate([[0], np.cumsum([e - s for s, e in sel])]).astype(np.int32)
    cat = lambda a: np.concatenate([a[s:e] for s, e in sel])
    return O.Spectra(offs, cat(mz), cat(it), cat(chg), pmz[list(rows)], pz[list(rows)])


def _check_against_oracle(O, sl, q, z, tol, mode, k, nprobe, res, key):
    part = sl.partitions[z]
    L = O.Spectra(*part.spectra.to('cpu').numpy())
    ivf = _host_ivf(O, part.index)
    q_pmz = q.numpy()[4].astype(np.float64)
    for i in range(q.n):
        keep = _window_mask(q_pmz[i], key, z, tol, mode)
        ref = O.search_batch(_spectra_rows(O, q, [i]), L, key, z, _filtered(O, ivf, keep), k, nprobe, tol, mode,
                             0.02, True, pm_stride=res.pm_pairs.shape[1], want_knn=True)
        assert np.array_equal(res.knn[i], ref['knn_I'][0]), i
        for f, g in (('n_candidates', 'n_cand'), ('best_row', 'best_row'), ('best_score', 'best_score'),
                     ('pm_count', 'pm_count')):
            assert getattr(res, f)[i] == ref[g][0], (f, i)
        n = res.pm_count[i]
        assert np.array_equal(res.pm_pairs[i, :n], ref['pm_pairs'][0, :n]), i


@pytest.fixture(scope='module')
def tie_world():
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib0, aux, lib = _tie_library()
    cfg = Config.open_search(num_list=16, num_probe=8, num_candidates=256, index='ivfpq', kmeans_niter=4)
    sl = SpectralLibrary(lib, config=cfg)
    idx = sl._get_ann_index(2)
    yield lib0, aux, lib, sl, idx
    sl.shutdown()


def test_index_level_matches_the_filtered_oracle(O, tie_world):
    lib0, aux, lib, sl, idx = tie_world
    ivf = _host_ivf(O, idx)
    q = _queries(lib0, aux, 48, seed=72, with_copies=8)
    xq = sl._encode(q.to(sl.device)).cpu().numpy()
    q_pmz = q.numpy()[4].astype(np.float64)
    key0 = np.ascontiguousarray(sl.partitions[2].precursor_mz, np.float32)
    key_nan = key0.copy()
    key_nan[::7] = np.nan
    for i in range(0, 2000, 97):      # the vectorised window test is precursor_ok
        for tol, mode in ((300.0, 'Da'), (2e5, 'ppm')):
            assert bool(_window_mask(q_pmz[0], key0[i:i + 1], 2, tol, mode)[0]) == \
                O.precursor_ok(q_pmz[0], key0[i], 2, tol, mode)
    cases = [(key0, 250.0, 'Da', 256), (key0, 2e5, 'ppm', 256), (key0, 10.0, 'ppm', 256), (key0, 2.0, 'Da', 64),
             (key0, -1.0, 'Da', 32), (key0, 1e9, 'Da', 256), (key_nan, 300.0, 'Da', 200), (key0, 300.0, 'Da', 1024)]
    short_rows = 0
    idx.nprobe = 8
    for key, tol, mode, k in cases:
        idx.set_window_key(key)
        D, I = idx.search_window(xq, k, q_pmz, 2, tol, mode)
        for i in range(len(xq)):
            keep = _window_mask(q_pmz[i], key, 2, tol, mode)
            rD, rI = _filtered(O, ivf, keep).search(xq[i:i + 1], k, 8)
            assert np.array_equal(I[i], rI[0]), (tol, mode, k, i)
            v = rI[0] >= 0
            assert np.array_equal(D[i][v].view(np.uint32), rD[0][v].view(np.uint32)), (tol, mode, k, i)
            assert keep[I[i][I[i] >= 0]].all()
            short_rows += int((I[i] < 0).any())
        if tol < 0:                   # the window passes nothing
            assert (I == -1).all()
        if tol == 1e9:                # the window passes everything: asl_index_search itself
            D2, I2 = idx.search(xq, k)
            assert np.array_equal(I, I2) and np.array_equal(D.view(np.uint32), D2.view(np.uint32))
    assert short_rows > 0
    # ties at the k-th score: the copies of row 0 fill the rows of the first queries beyond k
    idx.set_window_key(key0)
    _, I = idx.search_window(xq[:8], 64, q_pmz[:8], 2, 250.0, 'Da')
    assert (I < 400).all() and (I >= 0).all()


@pytest.mark.parametrize('tol,mode', [(250.0, 'Da'), (2e5, 'ppm'), (0.5, 'Da')])
def test_fused_path_matches_the_filtered_oracle(O, tol, mode):
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib0, aux, lib = _tie_library()
    q = _queries(lib0, aux, 120, seed=73, with_copies=6)
    cfg = Config.open_search(num_list=16, num_probe=8, num_candidates=256, index='ivfpq', kmeans_niter=4,
                             precursor_tolerance_mass_open=tol, precursor_tolerance_mode_open=mode, ann_window='pre')
    sl = SpectralLibrary(lib, config=cfg)
    try:
        res = sl._search_batch(q, 2, 'open', want_knn=True)
        _check_against_oracle(O, sl, q, 2, tol, mode, 256, 8, res, sl.partitions[2].precursor_mz)
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
    finally:
        sl.shutdown()


def test_whole_window_equals_post():
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib0, aux, lib = _tie_library()
    q = _queries(lib0, aux, 150, seed=74, with_copies=4)
    out = {}
    for w in ('post', 'pre'):
        cfg = Config.open_search(num_list=16, num_probe=8, num_candidates=256, index='ivfpq', kmeans_niter=4,
                                 precursor_tolerance_mass_open=1e9, ann_window=w)
        sl = SpectralLibrary(lib, config=cfg)
        out[w] = (sl._search_batch(q, 2, 'open', want_knn=True), sl._search_batch(q, 2, 'open'))
        sl.shutdown()
    for a, b in zip(out['post'], out['pre']):
        for f in FIELDS:
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(out['post'][0].knn, out['pre'][0].knn)


def test_pre_keeps_every_in_window_candidate_of_post():
    from ann_solo_amd import synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, aux = synthetic.make_library(20000, seed=75, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, 256, seed=76, charge=2)
    cfg = Config.open_search(num_list=64, num_probe=16, num_candidates=256, index='ivfpq', kmeans_niter=4,
                             precursor_tolerance_mass_open=100.0)
    sl = SpectralLibrary(lib, config=cfg)
    try:
        idx = sl._get_ann_index(2)
        key = np.ascontiguousarray(sl.partitions[2].precursor_mz, np.float32)
        idx.set_window_key(key)
        xq = sl._encode(q.to(sl.device)).cpu().numpy()
        q_pmz = q.numpy()[4].astype(np.float64)
        _, I_post = idx.search(xq, 256)
        _, I_pre = idx.search_window(xq, 256, q_pmz, 2, 100.0, 'Da')
        grew = 0
        for i in range(len(xq)):
            ids = I_post[i][I_post[i] >= 0]
            kept = ids[_window_mask(q_pmz[i], key[ids], 2, 100.0, 'Da')]
            pre = set(I_pre[i][I_pre[i] >= 0].tolist())
            assert set(kept.tolist()) <= pre, i
            grew += len(pre) > len(kept)
        assert grew > len(xq) // 2         # the rows fill up where post's are mostly out of the window
    finally:
        sl.shutdown()


def test_key_follows_the_library_handle(O):
    """An index searched with library A, then -- same handle -- with library B created after A was
    freed (same size, precursors +40 Da): the window key must be B's."""
    from ann_solo_amd.packed import PackedSpectra
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib0, aux, libA = _tie_library()
    o, mz, it, chg, pmz, pz = libA.numpy()
    libB = PackedSpectra.from_numpy(o, mz, it, chg, np.asarray(pmz, np.float64) + 40.0, pz)
    q = _queries(lib0, aux, 80, seed=77)
    cfg = Config.open_search(num_list=16, num_probe=8, num_candidates=256, index='ivfpq', kmeans_niter=4,
                             precursor_tolerance_mass_open=60.0, ann_window='pre')
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
        _check_against_oracle(O, slB, q, 2, 60.0, 'Da', 256, 8, resB, slB.partitions[2].precursor_mz)
    finally:
        slB.shutdown()


def test_unsupported_cases_are_errors():
    from ann_solo_amd import _lib, faiss_compat as faiss, synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    L = _lib.lib()
    lib, aux = synthetic.make_library(3000, seed=78, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, 16, seed=79, charge=2)
    sl = SpectralLibrary(lib, config=Config.open_search(num_list=8, num_probe=4, num_candidates=64, index='ivfflat',
                                                         kmeans_niter=3))
    try:
        flat = sl._get_ann_index(2)
        xq = sl._encode(q.to(sl.device)).cpu().numpy()
        q_pmz = q.numpy()[4].astype(np.float64)
        key = np.ascontiguousarray(sl.partitions[2].precursor_mz, np.float32)
        assert L.asl_index_set_window_scan(flat._h, 1) == -3            # ASL_ERR_STATE
        assert L.asl_index_set_window_key(flat._h, len(key), _lib.ptr(key)) == -3
        with pytest.raises(_lib.AnnSoloMiError):
            flat.search_window(xq, 16, q_pmz, 2, 300.0)
        assert L.asl_index_set_window_scan(flat._h, 0) == 0
    finally:
        sl.shutdown()
    rng = np.random.default_rng(3)
    x = np.zeros((3000, 800), np.float32)
    for i in range(len(x)):
        x[i, rng.choice(800, 20, replace=False)] = rng.random(20)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    pq = faiss.IndexIVFPQ(faiss.IndexFlatIP(800), 800, 8, 32, 8)
    pq.train(x)
    pq.add(x)
    keyx = np.linspace(400, 1400, len(x)).astype(np.float32)
    pq.set_window_key(keyx)
    pq.nprobe = 4
    qk = keyx[:8].astype(np.float64)
    D, I = pq.search_window(x[:8], 16, qk, 2, 50.0)
    assert (I[:, 0] >= 0).all()
    pq.set_scan_variant(1)                      # the generic kernel: no window scan
    with pytest.raises(_lib.AnnSoloMiError):
        pq.search_window(x[:8], 16, qk, 2, 50.0)
    pq.set_scan_variant(0)
    with pytest.raises(_lib.AnnSoloMiError):    # k above the tiled set-mode limit
        pq.search_window(x[:8], 1281, qk, 2, 50.0)
    pq.shard(0, 2)                              # a sharded index
    assert L.asl_index_set_window_scan(pq._h, 1) == -3
    with pytest.raises(_lib.AnnSoloMiError):
        pq.search_window(x[:8], 16, qk, 2, 50.0)
    with pytest.raises(ValueError):
        Config.open_search(index='ivfflat', ann_window='pre')
    with pytest.raises(ValueError):
        Config.open_search(index='ivfpq', num_gpus=2, ann_window='pre')
    with pytest.raises(ValueError):
        Config.open_search(index='ivfpq', refine_k=512, ann_window='pre')
    s2 = SpectralLibrary(lib, config=Config.open_search(num_list=8, num_probe=4, num_candidates=64, index='ivfpq',
                                                         kmeans_niter=3, ann_window='pre'))
    try:
        with pytest.raises(ValueError):
            s2.enable_sharding()
    finally:
        s2.shutdown()
