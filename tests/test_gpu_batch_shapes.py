"""Every per-query entry point at odd batch sizes and mixes (cases: tests/batch_cases.py; what they reach:
tests/test_batch_cases_cpu.py). A query's answer must not depend on its neighbours, its position or the
batch size, yet the coarse quantiser's gate, the row chunks behind the 1 GiB score workspace, the
rescoring's list split and the encoder's workgroups are all chosen from the batch.

One method throughout: a small pool of items, each item's expected output computed ONCE with the oracle
(never with another device path), many batches gathered from the pool with replacement, every row of
every batch compared with its item's expectation as bits -- ids exact, no tolerances."""
import numpy as np
import pytest
import torch      # before the library's first HIP call: loaded later, torch's own HIP runtime finds no device

import batch_cases as BC
from selector_ref import assert_rows_equal, host_ivf

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------ 1. coarse scores under every gate outcome
@pytest.mark.parametrize('nlist', BC.COARSE_NLISTS)
def test_coarse_scores_of_a_row_do_not_depend_on_the_batch(O, nlist):
    """The whole ordered row of every list's score (nprobe = nlist), at every outcome of the device-side gate
    `n_over > m / 64`: the sparse DPP kernel alone, the sparse kernel walking its one dense row, the MFMA GEMM;
    m below 64, on it and one above; partial groups of 4 rows; nlist = 33: scalar tile loads and stores."""
    from ann_solo_amd import faiss_compat as faiss
    cen = BC.coarse_centroids(nlist)
    pool, dense = BC.coarse_pool()
    want_D, want_I = O.flat_search(cen, pool, nlist)
    idx = faiss.IndexIVFFlat(faiss.IndexFlatIP(BC.COARSE_D), BC.COARSE_D, nlist)
    idx.set_trained(cen)
    idx.set_scan_variant(0)
    for m, n_dense, take in BC.coarse_batches(dense):
        D, I = idx.coarse(pool[take], nlist)
        what = (nlist, m, n_dense)
        assert D.shape == (m, nlist) and np.array_equal(I, want_I[take]), what
        assert np.array_equal(_bits(D), _bits(want_D[take])), what


# ------------------------------------------------------------------ 2. index search at odd batch sizes
@pytest.fixture(scope='module')
def index_data(O):
    xb, pool, dense = BC.index_vectors(O)
    return xb, pool, BC.index_batches(dense)


def _assert_same_sets(got, want, what):
    """Unordered rows: the same (id, score bits) as the ordered expectation, padding last."""
    (D, I), (wD, wI) = got, want
    for r in range(len(wI)):
        n = int((wI[r] >= 0).sum())
        assert (I[r, :n] >= 0).all() and (I[r, n:] == -1).all(), (what, r)
        o, wo = np.argsort(I[r, :n]), np.argsort(wI[r, :n])
        assert np.array_equal(I[r, :n][o], wI[r, :n][wo]), (what, r)
        assert np.array_equal(_bits(D[r, :n][o]), _bits(wD[r, :n][wo])), (what, r)


@pytest.mark.parametrize('kind', BC.INDEX_KINDS)
def test_index_search_of_a_row_does_not_depend_on_the_batch(O, index_data, kind):
    """IndexFlatIP, IVF-Flat over float and over fixed-point postings, IVF-PQ (tiled scan) at 1 .. 257 rows:
    batches so dense that the coarse gate picks the GEMM, and batches with exactly m / 64 dense rows, which
    the scans search from their dense rows while the others come as entry lists. Ordered rows as bits;
    unordered rows as sets."""
    from ann_solo_amd import faiss_compat as faiss
    xb, pool, batches = index_data
    k, nprobe = BC.INDEX_K, BC.INDEX_NPROBE
    if kind == 'flat':
        idx = faiss.IndexFlatIP(800)
    elif kind == 'ivfpq':
        idx = faiss.IndexIVFPQ(faiss.IndexFlatIP(800), 800, BC.INDEX_NLIST, 32, 8)
    else:
        idx = faiss.IndexIVFFlat(faiss.IndexFlatIP(800), 800, BC.INDEX_NLIST, storage=kind[-4:])
    if kind != 'flat':
        idx.set_niter(BC.INDEX_NITER)
        idx.train(xb)
    idx.add(xb)
    idx.nprobe = nprobe
    if kind.startswith('ivfflat'):
        assert idx.flat_layout == (2 if kind.endswith('fx22') else 1)
    want = O.flat_search(xb, pool, k) if kind == 'flat' else host_ivf(O, idx).search(pool, k, nprobe)
    assert (want[1] >= 0).all()
    for size, draw, take in batches:
        assert_rows_equal(idx.search(pool[take], k), (want[0][take], want[1][take]), (kind, size, draw))
    idx.set_unordered(1)
    try:
        for size, draw, take in batches:
            _assert_same_sets(idx.search(pool[take], k), (want[0][take], want[1][take]), (kind, size, draw))
    finally:
        idx.set_unordered(0)


# ------------------------------------------------------------------ 3. the chunk loops at 1 GiB
@pytest.fixture(scope='module')
def chunk_data():
    return BC.chunk_vectors()


@pytest.fixture(scope='module')
def chunk_flat(chunk_data):
    from ann_solo_amd import faiss_compat as faiss
    idx = faiss.IndexFlatIP(BC.CHUNK_D)
    idx.add(chunk_data[0])
    return idx


@pytest.mark.parametrize('nq,k', BC.CHUNK_FLAT)
def test_flat_search_beyond_one_score_chunk(O, chunk_data, chunk_flat, nq, k):
    """2^18 vectors: a score row is 1 MiB, a chunk 1 024 rows. Queries periodic over 37 items, so a row that
    took another chunk's output slot or pass bound would hold another item's answer. k = 2 058: the bounded
    second pass (`upper + r0`)."""
    xb, pool = chunk_data
    want_D, want_I = O.flat_search(xb, pool, k)
    item = np.arange(nq) % BC.CHUNK_POOL
    assert_rows_equal(chunk_flat.search(BC.periodic(pool, nq), k), (want_D[item], want_I[item]), (nq, k))


def test_ivfflat_gemm_and_bitmap_beyond_one_score_chunk(O, chunk_data):
    """The dense formulation of IVF-Flat (scan variant 1): the probe bitmap of a row of the second chunk."""
    from ann_solo_amd import faiss_compat as faiss
    xb, pool = chunk_data
    c = BC.CHUNK_IVF
    idx = faiss.IndexIVFFlat(faiss.IndexFlatIP(BC.CHUNK_D), BC.CHUNK_D, c['nlist'])
    idx.set_trained(np.random.default_rng(7501).standard_normal((c['nlist'], BC.CHUNK_D)).astype(np.float32))
    idx.add(xb)
    idx.set_scan_variant(1)
    idx.nprobe = c['nprobe']
    want_D, want_I = host_ivf(O, idx).search(pool, c['k'], c['nprobe'])
    item = np.arange(c['nq']) % BC.CHUNK_POOL
    assert len({want_I[i].tobytes() for i in range(BC.CHUNK_POOL)}) == BC.CHUNK_POOL
    assert_rows_equal(idx.search(BC.periodic(pool, c['nq']), c['k']), (want_D[item], want_I[item]))


def test_coarse_quantiser_beyond_one_score_chunk(O):
    """4 096 lists: a chunk of the coarse scores is 65 536 rows; 65 537 queries make a second chunk of one row.
    `coarse` (its output offsets) and `search` over postings: the coarse stage's own entry lists hold the last
    chunk only, so the scan has to list the queries itself."""
    from ann_solo_amd import faiss_compat as faiss
    c = BC.CLOOP
    cen, xb, pool = BC.cloop_vectors()
    idx = faiss.IndexIVFFlat(faiss.IndexFlatIP(c['d']), c['d'], c['nlist'])
    idx.set_trained(cen)
    idx.add(xb)
    assert idx.flat_layout != 0
    idx.nprobe = c['nprobe']
    xq = BC.periodic(pool, c['nq'])
    item = np.arange(c['nq']) % BC.CHUNK_POOL
    want_D, want_I = O.coarse(pool, cen, c['nprobe'])
    D, I = idx.coarse(xq, c['nprobe'])
    assert np.array_equal(I, want_I[item]) and np.array_equal(_bits(D), _bits(want_D[item]))
    want = host_ivf(O, idx).search(pool, c['k'], c['nprobe'])
    assert (want[1] >= 0).sum() > 5 * BC.CHUNK_POOL
    assert_rows_equal(idx.search(xq, c['k']), (want[0][item], want[1][item]))


# ------------------------------------------------------------------ 4. rescoring with split lists
class _RescorePool:
    """Library, pool and -- per tolerance, computed once -- S[q, r]: the oracle's score of every (query, row);
    the oracle's match list of a (query, row) when a winner needs it."""

    def __init__(self, O):
        from ann_solo_amd.packed import PackedSpectra
        from score_hist_ref import pair_scores
        self.O = O
        self.lib_np, self.pool_np = BC.rescore_spectra()
        self.lib = PackedSpectra.from_numpy(*self.lib_np)
        self.Q, self.L = O.Spectra(*self.pool_np), O.Spectra(*self.lib_np)
        self.S = {tol: np.stack([pair_scores(O, self.Q, q, self.L, np.arange(BC.RS_NLIB), tol, True)
                                 for q in range(BC.RS_NPOOL)]) for tol in (BC.RS_TOL, 0.0)}
        self._matches = {}

    def matches(self, tol, q, row):
        key = (tol, int(q), int(row))
        if key not in self._matches:
            _, s, m = self.O.best_match(self.Q, int(q), self.L, np.array([row], np.int64), tol, True)
            assert s == self.S[tol][q, row]
            self._matches[key] = m
        return self._matches[key]

    def queries(self, item):
        from ann_solo_amd.packed import PackedSpectra
        return PackedSpectra.from_numpy(*BC.gather_spectra(self.pool_np, item))


@pytest.fixture(scope='module')
def rescore_pool(O):
    return _RescorePool(O)


def _check_winners(P, tol, item, rows, off, res):
    """numpy's answer from S: the first position of the largest score of the list."""
    best, score, count, pairs = res
    S = P.S[tol]
    for q in range(len(item)):
        c = rows[off[q]:off[q + 1]]
        if not len(c):
            assert best[q] == -1 and score[q] == 0.0 and count[q] == 0, q
            continue
        s = S[item[q], c]
        p = int(np.argmax(s))
        assert best[q] == p, (q, int(best[q]), p)
        assert _bits(score[q:q + 1])[0] == _bits(s[p:p + 1])[0], q
        m = P.matches(tol, item[q], c[p])
        assert count[q] == len(m) and pairs[q, :len(m)].tolist() == m.tolist(), q


@pytest.mark.parametrize('tol,ci', [(BC.RS_TOL, ci) for ci in range(len(BC.RS_CASES))] +
                         [(0.0, ci) for ci in BC.RS_TOL0_CASES])
def test_rescoring_on_both_sides_of_the_list_split(rescore_pool, tol, ci):
    """ysplit = min(64, cdiv(avg, 4096)) blocks per query when nq < 2048 and avg > 4096: lists of 4 096 | 4 097
    slots, 2 047 | 2 048 queries, the cap of 64, an empty list inside a split batch, and the first of three
    equal maxima that three different blocks see. Lists repeat rows."""
    from ann_solo_amd import spectrum_match
    P = rescore_pool
    item, rows, off = BC.rescore_case(ci, P.S[tol])
    assert BC.ysplit(len(item), len(rows)) == BC.RS_YSPLIT[ci]
    res = spectrum_match.rescore_batch(P.queries(item), P.lib, rows, off, tol, True)
    _check_winners(P, tol, item, rows, off, res)


@pytest.mark.parametrize('tol,ci', [(BC.RS_TOL, ci) for ci in BC.RS_TOPN_CASES] +
                         [(0.0, ci) for ci in BC.RS_TOL0_CASES])
def test_ranked_rescoring_on_both_sides_of_the_list_split(rescore_pool, tol, ci):
    """The same lists through asl_rescore_batch_topn, n_best = 3: a stable sort by (-score, position)."""
    from ann_solo_amd import spectrum_match
    P = rescore_pool
    item, rows, off = BC.rescore_case(ci, P.S[tol])
    best, score, count, pairs = spectrum_match.rescore_batch_topn(P.queries(item), P.lib, rows, off, tol, True, 3)
    for q in range(len(item)):
        c = rows[off[q]:off[q + 1]]
        s = P.S[tol][item[q], c]
        order = np.argsort(-s, kind='stable')[:3]
        for r in range(3):
            if r >= len(order):
                assert best[q, r] == -1 and score[q, r] == 0.0 and count[q, r] == 0, (q, r)
                continue
            p = int(order[r])
            assert best[q, r] == p, (q, r, int(best[q, r]), p)
            assert _bits(score[q, r:r + 1])[0] == _bits(s[p:p + 1])[0], (q, r)
            m = P.matches(tol, item[q], c[p])
            assert count[q, r] == len(m) and pairs[q, r, :len(m)].tolist() == m.tolist(), (q, r)


# ------------------------------------------------------------------ 5. encoder and the fused call
def test_encoder_of_a_spectrum_does_not_depend_on_the_batch(O):
    """ENC_WAVES = 4 spectra per workgroup: batches of 1 .. 9 spectra drawn from a pool with an empty spectrum,
    1, 2, 63, 64, 65 and 200 peaks and colliding bins; the dense rows and the entry lists."""
    from ann_solo_amd import _lib, spectrum
    pool = BC.encoder_pool()
    for norm in (True, False):
        want = O.encode_batch(pool[1], pool[2], pool[0], 10.96, 0.04, 800, 42, norm)
        for items in BC.encoder_batches():
            off, mz, inten = BC.gather_peaks(pool, items)
            n = len(items)
            got = spectrum.spectra_to_vectors(mz, inten, off, 11, 2010, 0.04, 800, norm)
            assert np.array_equal(_bits(got), _bits(want[items])), (norm, items)
            ent = torch.full((n, 64, 2), -1, dtype=torch.int32, device='cuda')
            cnt = torch.full((n,), -99, dtype=torch.int32, device='cuda')
            over = torch.zeros(1, dtype=torch.int32, device='cuda')
            _lib.check(_lib.lib().asl_encode_entries_batch(_lib.ptr(mz), _lib.ptr(inten), _lib.ptr(off), n, -1, 10.96,
                                                           0.04, 800, 42, int(norm), _lib.ptr(ent), _lib.ptr(cnt),
                                                           _lib.ptr(over)))
            ent, cnt = ent.cpu().numpy(), cnt.cpu().numpy()
            n_over = 0
            for r, it in enumerate(items):
                nz = np.nonzero(want[it])[0]
                if len(nz) > 64:
                    assert cnt[r] == -1 - len(nz), (norm, items, r)
                    n_over += 1
                    nz = nz[:64]
                else:
                    assert cnt[r] == len(nz), (norm, items, r)
                assert np.array_equal(ent[r, :len(nz), 0], nz * 128), (norm, items, r)
                assert np.array_equal(ent[r, :len(nz), 1], want[it, nz].view(np.int32)), (norm, items, r)
                assert not ent[r, len(nz):].any(), (norm, items, r)
            assert int(over.item()) == n_over, (norm, items)


@pytest.fixture(scope='module')
def fused_data():
    from ann_solo_amd import synthetic
    lib, aux = synthetic.make_library(3000, seed=7950, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, 48, seed=7951, charge=2)
    return lib, q


@pytest.mark.parametrize('index', ['ivfpq', 'ivfflat'])
def test_fused_search_at_odd_batch_sizes(O, fused_data, index):
    """SpectralLibrary._search_batch at 1, 3, 65 and 129 queries drawn from a pool of 48: per query, the
    precursor window over the returned neighbours, then the oracle's best match among them."""
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, pool = fused_data
    cfg = Config.open_search(num_list=16, num_probe=6, num_candidates=128, index=index, kmeans_niter=4,
                             precursor_tolerance_mass_open=500, precursor_tolerance_mode_open='Da')
    sl = SpectralLibrary(lib, config=cfg)
    try:
        L, Q = O.Spectra(*lib.numpy()), O.Spectra(*pool.numpy())
        pmz32 = lib.precursor_mz.numpy().astype(np.float32)
        qpmz = pool.precursor_mz.numpy()
        rng = np.random.default_rng(7952)
        seen, cache = {}, {}
        for nq in BC.FUSED_SIZES:
            items = rng.integers(0, pool.n, nq)
            res = sl._search_batch(pool.select(items), 2, 'open', want_knn=True)
            for i, it in enumerate(items.tolist()):
                knn = res.knn[i]
                # (the neighbour list of an item is the same whatever batch it came in)
                assert seen.setdefault(it, knn.tobytes()) == knn.tobytes(), (nq, i, it)
                if it not in cache:
                    cand = np.sort(np.array([r for r in knn if r >= 0 and O.precursor_ok(
                        float(qpmz[it]), pmz32[r], 2, 500, 'Da')], np.int64))
                    cache[it] = (cand,) + tuple(O.best_match(Q, it, L, cand, 0.02, True)[:2])
                cand, b, s = cache[it]
                assert res.n_candidates[i] == len(cand), (nq, i, it)
                if b < 0:
                    assert res.best_row[i] == -1, (nq, i, it)
                else:
                    assert res.best_row[i] == cand[b] and res.best_score[i] == s, (nq, i, it)
        assert len(seen) > 40
    finally:
        sl.shutdown()
