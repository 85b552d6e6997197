"""The short-row selection (`wave_select_kernel`, ivf_kernels.hip: one wave per score row, four rows a
workgroup) against the oracle, ids and score bits. Every case goes through `faiss_compat.IndexFlatIP(d).search`,
which reaches that kernel for ntotal <= 4096 and k <= 256; its score rows have ld = ntotal, so with ntotal not a
multiple of 4 every second row starts off a 16-byte boundary."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = (1, 2, 127, 128, 129, 255, 256)


def _check(O, xb, xq, ks, what):
    from ann_solo_amd import faiss_compat as faiss
    n = len(xb)
    idx = faiss.IndexFlatIP(xb.shape[1])
    idx.add(xb)
    for k in ks:
        Do, Io = O.flat_search(xb, xq, k)
        D, I = idx.search(xq, k)
        valid = Io >= 0
        assert valid.sum() == len(xq) * min(k, n), (what, k)
        assert np.array_equal(I, Io), (what, k, np.argwhere(I != Io)[:4])
        assert np.array_equal(D.view(np.uint32)[valid], Do.view(np.uint32)[valid]), (what, k)
        assert (I[:, n:] == -1).all(), (what, k)


@pytest.mark.parametrize('nq', [1, 3, 4, 5, 63, 257])
def test_row_counts(O, nq):
    """Idle waves of the last workgroup (a row count that is no multiple of four) and more than one workgroup."""
    rng = np.random.default_rng(nq)
    xb = rng.standard_normal((301, 2)).astype(np.float32)
    xq = rng.standard_normal((nq, 2)).astype(np.float32)
    _check(O, xb, xq, (1, 10, 128), ('rows', nq))


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 255, 256, 257, 4093, 4095, 4096])
def test_row_lengths_and_k(O, n):
    """Row lengths around the wave, the 16-byte chunk, the narrow kernel's 1 024 and the full row, crossed with k
    around the sort sizes; k > n pads with -1. Five rows: at n not a multiple of 4 they start at every offset
    inside a 16-byte line."""
    rng = np.random.default_rng(n)
    xb = rng.standard_normal((n, 2)).astype(np.float32)
    xq = rng.standard_normal((5, 2)).astype(np.float32)
    _check(O, xb, xq, KS, ('length', n))


def _tie_rows(case, n, rng):
    xb = np.zeros((n, 2), np.float32)
    if case == 'constant':
        xb[:, 0] = 3.5
        xq = np.array([[1, 0], [2, 5], [-1, 0], [0, 0]], np.float32)
        ks = (1, 7, 128, 256)
    elif case == 'two_values':
        # the k-th place lies inside the larger group: the lowest ids of the tie fill the row. n = 4096: 100 x 2.0,
        # the rest 1.0, k = 128 takes the 28 lowest ids of the 1.0s; n = 100: 40 x 2.0, k = 50 takes 10 of them
        big = 100 if n >= 1000 else 40
        xb[:, 0] = 1.0
        xb[rng.permutation(n)[:big], 0] = 2.0
        xq = np.array([[1, 0], [-1, 0], [3, 1]], np.float32)
        ks = (128, 50, 1, 256)
    elif case == 'ulps':
        # more than 512 distinct scores in the threshold bucket cannot be had from a handful of ulps alone: a
        # far outlier stretches [lo, hi], so the +-600 ulps around 37 all fall into one bucket of 512
        base = np.float32(37.0).view(np.int32)
        xb[:, 0] = (base + rng.integers(-600, 601, n).astype(np.int32)).view(np.float32)
        xb[n // 2, 0] = -1.0e6
        xq = np.array([[1, 0], [-1, 0], [1, 9]], np.float32)
        ks = (1, 7, 128, 256)
    elif case == 'few_ulps':
        base = np.float32(37.0).view(np.int32)
        xb[:, 0] = (base + rng.integers(-3, 4, n).astype(np.int32)).view(np.float32)
        xq = np.array([[1, 0], [-1, 0], [1, 9]], np.float32)
        ks = (1, 7, 128, 256)
    else:                                        # hi - lo overflows fp32, every score stays finite
        xb[:, 0] = (rng.choice([-1.0, 1.0], n) * (0.5 + 0.5 * rng.random(n)) * 1.8e19).astype(np.float32)
        xb[:, 1] = rng.standard_normal(n).astype(np.float32)
        xq = np.array([[1.8e19, 0], [-1.8e19, 1], [1.8e19, -3]], np.float32)
        ks = (1, 7, 128, 256)
    return xb, xq, ks


@pytest.mark.parametrize('n', [100, 4096])
@pytest.mark.parametrize('case', ['constant', 'two_values', 'ulps', 'few_ulps', 'overflow'])
def test_tie_shapes(O, case, n):
    """Rows whose threshold bucket is overfull or whose range is degenerate: the key passes inside the wave."""
    xb, xq, ks = _tie_rows(case, n, np.random.default_rng(n + len(case)))
    if case == 'ulps' and n == 4096:      # the shape is what it claims: > 512 distinct scores within 1/511 of the range
        s = np.unique(xb[:, 0][xb[:, 0] > 0])
        assert len(s) > 512 and (s.max() - s.min()) * 511 < s.max() + 1.0e6
    if case == 'overflow':
        row = O.flat_search(xb, xq[:1], n)[0][0]
        with np.errstate(over='ignore'):
            assert np.isinf(np.float32(row.max()) - np.float32(row.min())) and np.isfinite(row).all()
    _check(O, xb, xq, ks, (case, n))


@pytest.mark.parametrize('n', [100, 4096])
def test_usual_and_tie_rows_in_one_workgroup(O, n):
    """Random and all-zero queries mixed so that the all-zero row (every score 0: the key passes) sits at wave
    position 0, 1, 2 and 3 of a workgroup in turn, beside three rows on the usual path; a workgroup of four tie
    rows and the partial last workgroup come with it."""
    rng = np.random.default_rng(7 * n)
    xb = rng.standard_normal((n, 64)).astype(np.float32)
    nq = 4 * 9 + 3
    xq = rng.standard_normal((nq, 64)).astype(np.float32)
    r = np.arange(nq)
    zero = (r % 4) == ((r // 4) % 4)
    zero[32:36] = True
    xq[zero] = 0.0
    assert zero[[0, 5, 10, 15]].all() and not zero[[1, 2, 3, 4]].any()
    _check(O, xb, xq, (1, 128, 256), ('mixed', n))


# ------------------------------------------------------------------ entry lists from the encoder
def _spectrum_with_nonzeros(O, rng, want):
    """(mz, intensity) of a spectrum whose encoded vector has exactly `want` non-zero components."""
    mz = np.sort(rng.uniform(100.0, 1900.0, want + 40)).astype(np.float32)
    it = (rng.random(len(mz)) + 0.05).astype(np.float32)
    for n in range(want, len(mz) + 1):
        v = O.encode_batch(mz[:n], it[:n], np.array([0, n], np.int32), 10.96, 0.04, 800)
        if np.count_nonzero(v[0]) == want:
            return mz[:n], it[:n]
    raise AssertionError('no prefix with %d non-zeros' % want)


def _replace(pack, items):
    """pack's arrays with the spectra of `items` ({row: (mz, intensity)}) put in place of its own."""
    o, mz, it, chg, pmz, pz = pack
    ms, is_, off = [], [], [0]
    for r in range(len(o) - 1):
        m, i = items.get(r, (mz[o[r]:o[r + 1]], it[o[r]:o[r + 1]]))
        ms.append(np.asarray(m, np.float32))
        is_.append(np.asarray(i, np.float32))
        off.append(off[-1] + len(m))
    return np.asarray(off, np.int32), np.concatenate(ms), np.concatenate(is_), None, pmz, pz


@pytest.fixture(scope='module')
def list_batches(O):
    """The library and two batches of 256 queries. `sparse`: one row with exactly 64 non-zeros, one with 65 (a
    single dense row: the sparse kernel keeps the batch and walks that row from its dense form) and one with a
    component that underflows to zero in the normalisation (a bin that holds a peak and is no entry). `dense`:
    eight rows with more than 64 non-zeros, more than nq / 64 = 4: the gate hands the batch to the dense GEMM.
    A row WITHOUT entries cannot leave this encoder: a vector of zeros is normalised to 0 / 0 in every component,
    oracle and device alike, so a spectrum without peaks is a row of 800 NaNs, not an empty list; the empty list is
    checked where it can occur, without normalisation (test_gpu_batch_shapes: the encoder's pool)."""
    from ann_solo_amd import synthetic
    from ann_solo_amd.packed import PackedSpectra
    lib, aux = synthetic.make_library(4000, seed=31, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, 256, seed=32, charge=2)
    rng = np.random.default_rng(33)
    s64, s65 = _spectrum_with_nonzeros(O, rng, 64), _spectrum_with_nonzeros(O, rng, 65)
    under = (np.array([300.0, 500.0, 700.0], np.float32), np.array([1e15, 1e-35, 3e14], np.float32))
    sparse = _replace(q.numpy(), {5: s64, 130: s65, 255: under})
    dense = _replace(q.numpy(), {r: _spectrum_with_nonzeros(O, rng, 66 + r % 7) for r in (0, 3, 64, 65, 100, 191, 192, 255)})
    for pack, n_dense in ((sparse, 1), (dense, 8)):
        v = O.encode_batch(pack[1], pack[2], pack[0], 10.96, 0.04, 800)
        assert (np.count_nonzero(v, axis=1) > 64).sum() == n_dense
    v = O.encode_batch(sparse[1], sparse[2], sparse[0], 10.96, 0.04, 800)
    assert np.count_nonzero(v[5]) == 64 and np.count_nonzero(v[130]) == 65
    assert np.count_nonzero(v[255]) == 2 and np.isfinite(v[255]).all()       # three bins hold a peak, two are entries
    return lib, PackedSpectra.from_numpy(*sparse), PackedSpectra.from_numpy(*dense)


@pytest.mark.parametrize('index', ['ivfpq', 'ivfflat'])
def test_entry_lists_from_the_encoder(O, list_batches, index, monkeypatch):
    """The unsharded search encodes the rows together with their entry lists and the coarse stage scores from
    those; ASL_COARSE_LISTS=0 keeps the lists rebuilt from the dense rows. Both routes give the same winners,
    scores, candidate counts and neighbour lists, synchronous and pipelined."""
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, sparse, dense = list_batches
    cfg = Config.open_search(num_list=16, num_probe=6, num_candidates=128, index=index, kmeans_niter=4,
                             precursor_tolerance_mass_open=500, precursor_tolerance_mode_open='Da')
    sl = SpectralLibrary(lib, config=cfg)
    try:
        for name, q in (('sparse', sparse), ('dense', dense)):
            got = {}
            for switch in ('1', '0'):
                monkeypatch.setenv('ASL_COARSE_LISTS', switch)
                res = sl._search_batch(q, 2, 'open', want_knn=True)
                sl.set_pipeline(True)
                a = sl._search_batch(q.to('cuda:0'), 2, 'open', device_out=True)
                b = sl._search_batch(q.to('cuda:0'), 2, 'open', device_out=True)
                sl.synchronize()
                sl.set_pipeline(False)
                for p in (a, b):
                    assert np.array_equal(p.best_row.cpu().numpy(), res.best_row), (name, switch)
                    assert np.array_equal(p.best_score.cpu().numpy().view(np.uint64),
                                          res.best_score.view(np.uint64)), (name, switch)
                got[switch] = res
            on, off = got['1'], got['0']
            assert np.array_equal(on.knn, off.knn), name
            assert np.array_equal(on.best_row, off.best_row), name
            assert np.array_equal(on.best_score.view(np.uint64), off.best_score.view(np.uint64)), name
            assert np.array_equal(on.n_candidates, off.n_candidates), name
            assert (on.knn[:, 0] >= 0).all(), name
    finally:
        sl.shutdown()
