"""The product quantiser against the oracle at every shape asl_index_create accepts: training
(coarse k-means, PQ k-means with its subsample and its empty-cluster split), encoding, the look-up
table and the ADC scan -- pq_m 4 .. 64, 1 .. 8 bits, sub-vectors on both sides of the register
path of the L2 kernels (dsub <= 32) and codebooks beyond one 64 KB round of LDS. Only pq_m = 32
with 8 bits and d <= 1020 takes the tiled scan (the last and the first d on either side of that are
tested); every other shape runs pq_scan_kernel<M> / adc_score<M>, the wide path of l2_argmin (the one
body of l2_assign_kernel / pq_encode_kernel: in one piece or in rounds), or both. Everything is compared bit for
bit: score and centroid bits as uint32, ids / codes / offsets as integers, no tolerance, ties
included (duplicated library vectors and all-zero queries force equal scores; the oracle and the
kernels both put the lowest id first)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NITER = 3
SEED = 4321
NLIST = 16

# (d, pq_m, pq_bits); d = 800 / 832: hashed spectra, small d: random dense vectors. pq_m = 64 does not
# divide the default hash length 800 (asl_index_create refuses it, see the refusals): its shapes run
# at the next multiple of 64, vectors hashed to 832 components.
SHAPES = [
    (800, 4, 8), (800, 8, 8), (800, 16, 8),   # wide training / encoding paths: dsub 200, 100 in rounds (204 800 / 102 400 B codebooks), 50 in one piece
    (832, 64, 8),                             # M = 64 scan (two terms per partial), the largest look-up table
    (800, 16, 4),                             # PQ training subsample: n > 16 * 256
    (800, 8, 6), (800, 32, 5),                # ksub < 256, also at the tiled kernel's own m
    (832, 64, 1), (800, 4, 2),                # extreme small shapes: rows of mostly tied scores
    (128, 4, 8),                              # dsub = 32: last register-path width
    (132, 4, 8),                              # dsub = 33: first wide-path width
    (64, 16, 8),                              # dsub = 4
]
SUBSAMPLED = [(800, 16, 4), (832, 64, 1), (800, 4, 2)]
DEEP_K = [(800, 16, 8), (800, 8, 6)]          # k beyond TK_MAX_K: bounded passes of pq_scan_kernel
LARGEST = (22464, 64, 8)                      # 16 384 + 22 464 = 38 848 floats: the widest d at the largest look-up table
TILED_EDGE = [(992, 32, 8), (1024, 32, 8)]      # pq_m = 32, 8 bits: the widest d of the tiled scan, the first beyond it
ids_of = lambda s: 'd%d-m%d-b%d' % s


def _hashed(O, d):
    """5 000 library vectors hashed to d components, 200 queries; 250 library rows are exact copies
    of others (50 of them of ONE vector) and three queries are all zero."""
    from ann_solo_amd import synthetic
    lib, aux = synthetic.make_library(5000, seed=131, device='cpu')
    q, _ = synthetic.make_queries(lib, aux, 200, seed=132)
    o, mz, inten, *_ = lib.numpy()
    xb = O.encode_batch(mz, inten, o, 10.96, 0.04, d)
    o, mz, inten, *_ = q.numpy()
    xq = O.encode_batch(mz, inten, o, 10.96, 0.04, d)
    xb[4000:4200] = xb[100:300]
    xb[4900:4950] = xb[7]
    xq[[5, 77, 199]] = 0.0
    xq[11] = xb[7]
    return xb, xq


def _dense(d):
    rng = np.random.default_rng(1000 + d)
    xb = rng.standard_normal((5000, d)).astype(np.float32)
    xq = rng.standard_normal((200, d)).astype(np.float32)
    xb[4000:4200] = xb[100:300]
    xb[4900:4950] = xb[7]
    xb[-300:] = np.round(xb[-300:])               # a coarse grid: equal sub-vector distances
    xq[[5, 77, 199]] = 0.0
    xq[11] = xb[7]
    return xb, xq


@pytest.fixture(scope='module')
def world(O):
    """shape -> the oracle's side of it, computed once: vectors, coarse centroids, codebooks, list
    assignment, codes and the inverted lists."""
    data, coarse, full = {}, {}, {}

    def get(shape):
        d, m, bits = shape
        if shape not in full:
            if d not in data:
                data[d] = _hashed(O, d) if d >= 800 else _dense(d)
            xb, xq = data[d]
            if d not in coarse:
                cen = O.kmeans(xb, NLIST, NITER, SEED, 0, 256)
                coarse[d] = cen, O.assign(xb, cen, 0)
            cen, a = coarse[d]
            cb = O.pq_train(xb, cen, m, 1 << bits, NITER, SEED + 7)
            codes = O.pq_encode(xb, cen, a, cb)
            full[shape] = dict(xb=xb, xq=xq, cen=cen, cb=cb, assign=a, codes=codes,
                               ivf=O.HostIVF(cen, a, codes, cb))
        return full[shape]
    return get


def _new_index(shape):
    from ann_solo_amd import faiss_compat as faiss
    d, m, bits = shape
    return faiss.IndexIVFPQ(faiss.IndexFlatIP(d), d, NLIST, m, bits)


@pytest.fixture(scope='module')
def filled():
    """shape -> an index holding the oracle's quantisers and the library (one per shape)."""
    made = {}

    def get(shape, w):
        if shape not in made:
            idx = _new_index(shape)
            idx.set_trained(w['cen'], w['cb'])
            idx.add(w['xb'])
            made[shape] = idx
        return made[shape]
    return get


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('shape', SHAPES, ids=ids_of)
def test_train_bit_exact(world, shape):
    d, m, bits = shape
    w = world(shape)
    xb = w['xb']
    if shape in SUBSAMPLED:
        assert len(xb) > (1 << bits) * 256         # pq_train_device takes the permutation subsample
    idx = _new_index(shape)
    i = idx.info()
    assert (i.pq_m, i.pq_ksub, i.pq_dsub) == (m, 1 << bits, d // m)
    idx.set_niter(NITER)
    idx.seed = SEED
    idx.train(xb)
    assert idx.is_trained
    assert np.array_equal(_bits(idx.centroids()), _bits(w['cen']))
    assert np.array_equal(_bits(idx.codebooks()), _bits(w['cb']))


@pytest.mark.parametrize('shape', SHAPES, ids=ids_of)
def test_encode_and_lists_bit_exact(world, shape):
    w = world(shape)
    xb, ivf = w['xb'], w['ivf']
    idx = _new_index(shape)
    idx.set_trained(w['cen'], w['cb'])
    idx.add(xb[:2100])
    idx.add(xb[2100:])                             # two add() calls: ids keep add order
    off, ids, codes = idx.lists()
    assert np.array_equal(off, ivf.list_offsets)
    assert np.array_equal(ids, ivf.ids)
    assert np.array_equal(codes, ivf.payload)
    assert int(codes.max()) < (1 << shape[2])


@pytest.mark.parametrize('by_residual', [True, False], ids=['by_residual', 'raw'])
@pytest.mark.parametrize('shape', [(128, 4, 8), (132, 4, 8), (800, 8, 8)], ids=ids_of)
def test_encode_blocks_of_one_live_lane_and_exactly_full(O, world, shape, by_residual):
    """Register path, one-piece wide path and rounds: the lanes of a block past the last vector stay with the
    block through the staging barriers and write nothing. add() of 1 vector (one live lane), of 256 (a block
    that is exactly full) and of 1 again: after each, the lists equal the oracle's over the same prefix."""
    import raw_pq_ref as R
    w = world(shape)
    xb, cen, cb, a = w['xb'][:258], w['cen'], w['cb'], w['assign']
    want = w['codes'] if by_residual else R.raw_codes(O, xb, cb)
    idx = _new_index(shape)
    if not by_residual:
        idx.by_residual = False
    idx.set_trained(cen, cb)
    n = 0
    for step in (1, 256, 1):
        idx.add(xb[n:n + step])
        n += step
        ivf = O.HostIVF(cen, a[:n], want[:n], cb)
        off, ids, codes = idx.lists()
        assert idx.ntotal == n
        assert np.array_equal(off, ivf.list_offsets), n
        assert np.array_equal(ids, ivf.ids), n
        assert np.array_equal(codes, ivf.payload), n
    assert n == 258


@pytest.mark.parametrize('shape', [(800, 8, 8), (132, 4, 8), (128, 4, 8)], ids=ids_of)
def test_encode_with_identical_codes_takes_the_lowest(O, world, shape):
    """Codebooks in which several codes are the same point (what a k-means that ends on duplicated
    data leaves): every vector nearest to such a point is equally far from all its copies, and the
    code is the lowest of them."""
    w = world(shape)
    cb = w['cb'].copy()
    ksub = cb.shape[1]
    cb[:, ksub - 1] = cb[:, 3]
    cb[:, ksub // 2] = cb[:, 3]
    cb[:, 9] = cb[:, 200]
    idx = _new_index(shape)
    idx.set_trained(w['cen'], cb)
    idx.add(w['xb'])
    want = O.pq_encode(w['xb'], w['cen'], w['assign'], cb)
    assert (want == 3).any() and (want == 9).any()
    assert not (want == ksub - 1).any() and not (want == ksub // 2).any() and not (want == 200).any()
    ivf = O.HostIVF(w['cen'], w['assign'], want, cb)
    off, ids, codes = idx.lists()
    assert np.array_equal(ids, ivf.ids)
    assert np.array_equal(codes, ivf.payload)


@pytest.mark.parametrize('shape', SHAPES, ids=ids_of)
def test_coarse_and_lut_bit_exact(O, world, filled, shape):
    w = world(shape)
    idx, xq = filled(shape, w), w['xq']
    for nprobe in (1, 4, 16, 99):
        D, I = idx.coarse(xq, nprobe)
        Do, Io = O.coarse(xq, w['cen'], min(nprobe, NLIST))
        assert np.array_equal(I, Io), nprobe
        assert np.array_equal(_bits(D), _bits(Do)), nprobe
    lut = idx.pq_lut(xq[:12])                       # row 5 is all zero, row 11 a library vector
    for i in range(12):
        assert np.array_equal(_bits(lut[i]), _bits(O.pq_lut(xq[i], w['cb']))), i


@pytest.mark.parametrize('shape', SHAPES, ids=ids_of)
def test_search_identical_to_oracle(world, filled, shape):
    from ann_solo_amd import _lib
    d, m, bits = shape
    w = world(shape)
    idx, ivf, xq = filled(shape, w), w['ivf'], w['xq']
    if m == 32:        # fewer than 8 bits: the tiled scan (and with it the packed-key rows) is not in use
        assert idx.info().pq_ksub == 1 << bits < 256
        assert _lib.lib().asl_index_supports_keys(idx._h, 200, 8) == 0
        assert _lib.lib().asl_index_supports_keys(_new_index((d, 32, 8))._h, 200, 8) == 1
    grid = [(k, nprobe) for nprobe in (1, 8, 16) for k in (1, 200, 1024)]
    if shape in DEEP_K:
        grid += [(3000, 16), (3000, 5)]
    padded = False
    for k, nprobe in grid:
        idx.nprobe = nprobe
        D, I = idx.search(xq, k)
        Do, Io = ivf.search(xq, k, nprobe)
        assert np.array_equal(I, Io), (k, nprobe)
        assert np.array_equal(_bits(D), _bits(Do)), (k, nprobe)
        padded |= bool((Io == -1).any())
    assert padded                                   # (1024, 1): a list holds fewer than k vectors
    # that the rows compared above hold the tie case at all, read off the oracle's own output (row 5 is an
    # all-zero query: 1 024 equal scores, ascending ids)
    Dz, Iz = ivf.search(xq[[5]], 1024, 16)
    assert (Dz == Dz[0, 0]).all() and (np.diff(Iz[0]) > 0).all()


@pytest.mark.parametrize('shape', TILED_EDGE, ids=ids_of)
def test_m32_8bit_on_both_sides_of_the_tiled_scan_limit(O, shape):
    """pq_m = 32 with 8 bits is the tiled scan's shape, but that kernel holds a query of at most 1020
    components. d = 992 is the widest multiple of 32 it takes; d = 1024 trains and encodes alike and is
    searched by the generic kernel with no setting of the caller's: both equal the oracle."""
    from ann_solo_amd import _lib, faiss_compat as faiss
    d, m, bits = shape
    rng = np.random.default_rng(d)
    xb = rng.standard_normal((1500, d)).astype(np.float32)
    xb[1400:1450] = xb[3]
    xq = rng.standard_normal((40, d)).astype(np.float32)
    xq[2] = 0.0
    xq[5] = xb[3]
    cen = O.kmeans(xb, 4, 1, SEED, 0, 256)
    cb = O.pq_train(xb, cen, m, 256, 1, SEED + 7)
    a = O.assign(xb, cen, 0)
    ivf = O.HostIVF(cen, a, O.pq_encode(xb, cen, a, cb), cb)
    idx = faiss.IndexIVFPQ(faiss.IndexFlatIP(d), d, 4, m, bits)
    idx.set_niter(1)
    idx.seed = SEED
    idx.train(xb)
    assert np.array_equal(_bits(idx.centroids()), _bits(cen))
    assert np.array_equal(_bits(idx.codebooks()), _bits(cb))
    idx.add(xb)
    off, ids, codes = idx.lists()
    assert np.array_equal(off, ivf.list_offsets) and np.array_equal(ids, ivf.ids)
    assert np.array_equal(codes, ivf.payload)
    assert _lib.lib().asl_index_supports_keys(idx._h, 200, 2) == int(d <= 1020)     # the tiled scan is / is not in use
    for k, nprobe in ((1, 1), (200, 2), (1024, 4), (1024, 1)):
        idx.nprobe = nprobe
        D, I = idx.search(xq, k)
        Do, Io = ivf.search(xq, k, nprobe)
        assert np.array_equal(I, Io), (k, nprobe)
        assert np.array_equal(_bits(D), _bits(Do)), (k, nprobe)


def test_the_largest_accepted_shape_trains_encodes_and_searches(O):
    """d = 22 464 with pq_m = 64, 8 bits: asl_index_create accepts nothing wider at this table size.
    Codebooks of 359 424 B are staged 46 codes at a time, the table kernel and the scan ask for
    155 392 B and 163 600 B of LDS. k = 257 needs the next top-k buffer and is refused by name."""
    from ann_solo_amd._lib import AnnSoloMiError
    d, m, bits = LARGEST
    rng = np.random.default_rng(22464)
    xb = rng.standard_normal((400, d)).astype(np.float32)
    xb[300:330] = xb[3]
    xq = rng.standard_normal((16, d)).astype(np.float32)
    xq[2] = 0.0
    cen = O.kmeans(xb, 2, 1, SEED, 0, 256)
    cb = O.pq_train(xb, cen, m, 256, 1, SEED + 7)
    a = O.assign(xb, cen, 0)
    ivf = O.HostIVF(cen, a, O.pq_encode(xb, cen, a, cb), cb)
    from ann_solo_amd import faiss_compat as faiss
    idx = faiss.IndexIVFPQ(faiss.IndexFlatIP(d), d, 2, m, bits)
    idx.set_niter(1)
    idx.seed = SEED
    idx.train(xb)
    assert np.array_equal(_bits(idx.centroids()), _bits(cen))
    assert np.array_equal(_bits(idx.codebooks()), _bits(cb))
    idx.add(xb)
    off, ids, codes = idx.lists()
    assert np.array_equal(off, ivf.list_offsets) and np.array_equal(ids, ivf.ids)
    assert np.array_equal(codes, ivf.payload)
    lut = idx.pq_lut(xq[:3])
    for i in range(3):
        assert np.array_equal(_bits(lut[i]), _bits(O.pq_lut(xq[i], cb)))
    for k, nprobe in ((1, 1), (100, 2), (256, 2), (256, 1)):
        idx.nprobe = nprobe
        D, I = idx.search(xq, k)
        Do, Io = ivf.search(xq, k, nprobe)
        assert np.array_equal(I, Io), (k, nprobe)
        assert np.array_equal(_bits(D), _bits(Do)), (k, nprobe)
    with pytest.raises(AnnSoloMiError) as e:
        idx.search(xq, 257)
    assert 'LDS' in str(e.value)


def test_pq_kmeans_empty_cluster_split(O):
    """PQ k-means on residual sub-vectors with fewer distinct values than codes (6 points repeated
    400 times, a 4-bit PQ): clusters run empty in every iteration and are refilled by the split of
    a populated one (centroid * (1 +- 1/1024), alternating by component)."""
    from ann_solo_amd import faiss_compat as faiss
    rng = np.random.default_rng(5)
    base = rng.random((6, 32)).astype(np.float32)
    x = np.repeat(base, 400, axis=0)               # 2400 points, 6 distinct
    x += (rng.random(x.shape) < 0.01).astype(np.float32) * 0.001
    cen = O.kmeans(x, 2, 4, SEED, 0, 256)
    cb = O.pq_train(x, cen, 4, 16, 4, SEED + 7)
    # the oracle did split in the last iteration: rows a, b = c * (1 + eps), c * (1 - eps) on the even
    # components and the other way round on the odd ones (fp32 products: 2^-22 of slack)
    eps = 1.0 / 1024.0
    want = np.where(np.arange(8) % 2 == 0, (1 + eps) / (1 - eps), (1 - eps) / (1 + eps))
    split = 0
    for mi in range(4):
        for a in range(16):
            for b in range(16):
                r = cb[mi, a].astype(np.float64) / np.where(cb[mi, b] != 0, cb[mi, b], np.nan).astype(np.float64)
                split += bool(np.all(np.abs(r / want - 1.0) < 2.0 ** -22))
    assert split > 0
    idx = faiss.IndexIVFPQ(faiss.IndexFlatIP(32), 32, 2, 4, 4)
    idx.set_niter(4)
    idx.seed = SEED
    idx.train(x)
    assert np.array_equal(_bits(idx.centroids()), _bits(cen))
    assert np.array_equal(_bits(idx.codebooks()), _bits(cb))


def test_save_and_load_of_a_generic_shape(world, tmp_path):
    from ann_solo_amd import faiss_compat as faiss
    shape = (800, 16, 4)
    w = world(shape)
    xq, ivf = w['xq'], w['ivf']
    idx = _new_index(shape)
    idx.set_trained(w['cen'], w['cb'])
    idx.add(w['xb'])
    idx.nprobe = 8
    D, I = idx.search(xq, 200)
    path = str(tmp_path / 'm16b4.idxmi')
    faiss.write_index(idx, path)
    back = faiss.read_index(path)
    i = back.info()
    assert (i.d, i.pq_m, i.pq_ksub, i.pq_dsub, i.ntotal) == (800, 16, 16, 50, len(w['xb'])) and back.is_trained
    assert np.array_equal(_bits(back.codebooks()), _bits(w['cb']))
    back.nprobe = 8
    D2, I2 = back.search(xq, 200)
    Do, Io = ivf.search(xq, 200, 8)
    assert np.array_equal(I2, I) and np.array_equal(_bits(D2), _bits(D))
    assert np.array_equal(I2, Io) and np.array_equal(_bits(D2), _bits(Do))


@pytest.mark.parametrize('k', [100, 512])
def test_refine_on_a_generic_shape(O, world, k):
    """The exact re-rank over the short-list of the generic scan (pq_m = 16): ids and exact scores
    equal the oracle's re-rank of the oracle's own 2k ADC candidates."""
    shape = (800, 16, 8)
    w = world(shape)
    xb, xq, ivf = w['xb'], w['xq'], w['ivf']
    idx = _new_index(shape)
    idx.set_refine(2 * k)                           # before add(): the exact rows are stored as vectors arrive
    idx.set_trained(w['cen'], w['cb'])
    idx.add(xb)
    for nprobe in (1, 6):
        idx.nprobe = nprobe
        D, I = idx.search(xq, k)
        _, I_short = ivf.search(xq, 2 * k, nprobe)
        Do, Io = O.refine(xb, xq, I_short, k)
        assert np.array_equal(I, Io), nprobe
        assert np.array_equal(_bits(D), _bits(Do)), nprobe


@pytest.mark.parametrize('pq', [dict(pq_m=16), dict(pq_m=32, pq_bits=6)], ids=['m16', 'm32-b6'])
def test_open_search_end_to_end_on_generic_shapes(O, pq):
    """SpectralLibrary's open search over an index of a generic PQ shape (trained and filled by the
    engine) against the oracle's search over the oracle's own quantisers, codes and lists: the
    neighbour rows, the winners, their scores and candidate counts. The generic scan takes no
    post-filter: the switch must change nothing."""
    from ann_solo_amd import _lib, synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, aux = synthetic.make_library(5000, seed=141, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, 200, seed=142, charge=2)
    cfg = Config.open_search(num_list=NLIST, num_probe=6, num_candidates=256, index='ivfpq', kmeans_niter=NITER,
                             seed=SEED, **pq)
    m, ksub = cfg.pq_m, 1 << cfg.pq_bits
    sl = SpectralLibrary(lib, config=cfg)
    L = _lib.lib()
    try:
        part = sl.partitions[2]
        o, mz, inten, *_ = part.spectra.to('cpu').numpy()
        xb = O.encode_batch(mz, inten, o, 10.96, 0.04, 800)
        cen = O.kmeans(xb, NLIST, NITER, SEED, 0, 256)
        cb = O.pq_train(xb, cen, m, ksub, NITER, SEED + 7)
        a = O.assign(xb, cen, 0)
        ivf = O.HostIVF(cen, a, O.pq_encode(xb, cen, a, cb), cb)
        i = sl._get_ann_index(2).info()
        assert (i.pq_m, i.pq_ksub) == (m, ksub)
        res = sl._search_batch(q, 2, 'open', want_knn=True)
        ref = O.search_batch(O.Spectra(*q.numpy()), O.Spectra(*part.spectra.to('cpu').numpy()), part.precursor_mz,
                             2, ivf, 256, 6, 300, 'Da', 0.02, True, pm_stride=res.pm_pairs.shape[1], want_knn=True)
        assert np.array_equal(res.knn, ref['knn_I'])                              # the candidate ids, in order
        assert (ref['best_row'] >= 0).mean() > 0.5
        for on in (0, 1):
            L.asl_set_scan_postfilter(on)
            for r in (sl._search_batch(q, 2, 'open'), sl._search_batch(q, 2, 'open', want_knn=True)):
                assert np.array_equal(r.best_row, ref['best_row']), on
                assert np.array_equal(r.best_score, ref['best_score']), on
                assert np.array_equal(r.n_candidates, ref['n_cand']), on
                assert np.array_equal(r.pm_count, ref['pm_count']), on
    finally:
        L.asl_set_scan_postfilter(1)
        sl.shutdown()


def test_refused_shapes_say_which_parameter(tmp_path):
    import struct
    from ann_solo_amd import _lib, faiss_compat as faiss
    from ann_solo_amd._lib import AnnSoloMiError
    err = lambda: (_lib.lib().asl_last_error() or b'').decode()
    for d, m, bits, word in ((96, 12, 8, 'pq_m=12'), (96, 3, 8, 'pq_m=3'), (800, 16, 9, 'pq_bits=9'),
                             (100, 8, 8, 'pq_m=8 does not divide d=100'), (800, 0, 8, 'pq_m=0'),
                             (800, 64, 8, 'pq_m=64 does not divide d=800')):
        with pytest.raises(AnnSoloMiError) as e:
            faiss.IndexIVFPQ(faiss.IndexFlatIP(d), d, NLIST, m, bits)
        assert word in str(e.value) and word in err(), (d, m, bits, str(e.value))
    # a query, its look-up table and the smallest top-k buffer (8 208 B) share a workgroup's 160 KB of LDS:
    # pq_m * 2^pq_bits + d <= 38 908 floats
    with pytest.raises(AnnSoloMiError) as e:
        faiss.IndexIVFPQ(faiss.IndexFlatIP(22528), 22528, NLIST, 64, 8)       # 16 384 + 22 528 = 38 912
    assert 'd=22528' in str(e.value) and 'LDS' in str(e.value) and '160 KB' in str(e.value)
    assert faiss.IndexIVFPQ(faiss.IndexFlatIP(LARGEST[0]), *LARGEST[:1], NLIST, *LARGEST[1:]).info().pq_dsub == 351
    # a file gets the same check as asl_index_create: the header of a good index, its d patched
    rng = np.random.default_rng(8)
    small = faiss.IndexIVFPQ(faiss.IndexFlatIP(64), 64, 2, 64, 8)
    small.set_niter(1)
    small.train(rng.standard_normal((300, 64)).astype(np.float32))
    path = str(tmp_path / 'wide.idxmi')
    faiss.write_index(small, path)
    assert faiss.read_index(path).info().pq_m == 64
    blob = bytearray(open(path, 'rb').read())
    blob[12:16] = struct.pack('<i', 22528)          # magic[8] version d ...
    open(path, 'wb').write(bytes(blob))
    with pytest.raises(AnnSoloMiError) as e:
        faiss.read_index(path)
    assert 'd=22528' in str(e.value) and 'LDS' in str(e.value)
    # fewer training vectors than codes
    rng = np.random.default_rng(9)
    idx = faiss.IndexIVFPQ(faiss.IndexFlatIP(64), 64, 4, 4, 8)
    with pytest.raises(AnnSoloMiError) as e:
        idx.train(rng.standard_normal((100, 64)).astype(np.float32))
    assert 'pq_bits' in str(e.value) and 'pq_bits' in err()
    assert not idx.is_trained
