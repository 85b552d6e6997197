"""The look-up addresses of the tiled IVF-PQ scan (csrc/pq_tile.hpp, lut_at / tile_adc): every code byte value
at every one of the 32 byte positions, against the oracle, ids and score bits equal, no tolerance.

The address of a table entry is made per look-up from one byte of a code word and the lane's column. What can go
wrong there is narrow -- a wrong byte position, a code of 128 or above (a select that sign-extends, a shift that
loses bit 7), an OR where an ADD was needed, a lane that reads a neighbour's column -- and trained data need not
hit it at every position, so the codes are made by hand: the codebooks are 256 pairwise distinct codewords per
sub-quantiser, a vector is its list's centroid plus the concatenation of chosen codewords, all on a dyadic grid, so
that the residual is the codeword exactly and the encoder must return the chosen code (distance 0, no ties).

Chosen codes: row i < 256 of the long list has c_m = (i + 37 m) mod 256, so every byte value occurs at every
position; then rows of all-0, all-255, all-127 and all-128; the rows of the short lists follow a second pattern.
List sizes 260, 1, 63, 64 and 65: partial, exact and several tiles. Queries: every table column live and distinct,
one live column, all zero, hashed spectra."""
import ctypes as C

import numpy as np
import pytest

D, M, NLIST = 800, 32, 5
DSUB = D // M
SIZES = [256 + 4, 1, 63, 64, 65]
N = sum(SIZES)
NQ = 8
Q_ALL_LIVE, Q_ONE_LIVE, Q_ZERO = 0, 1, 2
KS = (64, 512)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _design():
    """(vectors, lists, codes, centroids, codebooks)."""
    rng = np.random.default_rng(20817)
    cb = (rng.integers(-32, 33, size=(M, 256, DSUB)) / 64.0).astype(np.float32)
    for m in range(M):
        assert len(np.unique(cb[m], axis=0)) == 256            # pairwise distinct codewords
    cen = (rng.integers(-32, 33, size=(NLIST, D)) / 64.0).astype(np.float32)
    m = np.arange(M)
    codes = np.empty((N, M), np.int64)
    i = np.arange(256)
    codes[:256] = (i[:, None] + 37 * m[None, :]) % 256
    codes[256], codes[257], codes[258], codes[259] = 0, 255, 127, 128
    r = np.arange(N - 260)
    codes[260:] = (5 * r[:, None] + 91 * m[None, :] + 3) % 256
    codes = codes.astype(np.uint8)
    assign = np.repeat(np.arange(NLIST, dtype=np.int32), SIZES)
    x = cen[assign].copy()
    for mm in range(M):
        x[:, mm * DSUB:(mm + 1) * DSUB] += cb[mm, codes[:, mm]]   # exact: multiples of 1/64 below 2
    # every byte value at every position, and the four constant rows
    for mm in range(M):
        assert len(np.unique(codes[:256, mm])) == 256
    # rows in an order that is not the lists' (the index and the oracle both sort them by list)
    perm = rng.permutation(N)
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


@pytest.fixture(scope='module')
def world(O):
    x, assign, codes, cen, cb = _design()
    # the design check, on the CPU: the oracle's encoder returns exactly the designed codes
    assert np.array_equal(O.pq_encode(x, cen, assign, cb), codes)
    ivf = O.HostIVF(cen, assign, codes, cb)
    xq = _queries(O)
    rows = {k: ivf.search(xq, k, NLIST) for k in KS}
    return dict(x=x, assign=assign, codes=codes, cen=cen, cb=cb, ivf=ivf, xq=xq, rows=rows)


def test_the_oracle_encodes_the_designed_codes(O, world):
    codes, assign = world['codes'], world['assign']
    long_list = codes[assign == 0]
    for m in range(M):
        assert len(np.unique(long_list[:, m])) == 256
    for v in (0, 255, 127, 128):
        assert (long_list == v).all(1).any()
    assert np.array_equal(np.diff(world['ivf'].list_offsets), SIZES)
    D512, I512 = world['rows'][512]
    assert ((I512 >= 0).sum(1) == N).all()                     # k = 512 holds every vector, -1 padded behind
    # every table column of the all-live query is live, and no two columns are equal
    lut = O.pq_lut(world['xq'][Q_ALL_LIVE], world['cb'])
    assert (lut != 0).any(1).all() and len(np.unique(lut, axis=0)) == M
    assert (O.pq_lut(world['xq'][Q_ONE_LIVE], world['cb']) != 0).any(1).sum() == 1


@pytest.fixture(scope='module')
def index(world):
    from ann_solo_amd import _lib
    from ann_solo_amd import faiss_compat as faiss
    idx = faiss.IndexIVFPQ(faiss.IndexFlatIP(D), D, NLIST, M, 8)
    idx.set_trained(world['cen'], world['cb'])
    x = np.ascontiguousarray(world['x'], np.float32)
    lists = np.ascontiguousarray(world['assign'], np.int32)
    _lib.check(_lib.lib().asl_index_add_preassigned(idx._h, C.c_int64(len(x)), x.ctypes.data_as(C.c_void_p),
                                                    lists.ctypes.data_as(C.c_void_p)))
    idx.nprobe = NLIST
    return idx


@pytest.mark.gpu
def test_the_index_holds_the_designed_codes(world, index):
    off, ids, codes = index.lists()
    ivf = world['ivf']
    assert np.array_equal(off, ivf.list_offsets) and np.array_equal(ids, ivf.ids)
    assert np.array_equal(codes, ivf.payload)
    assert np.array_equal(codes, world['codes'][ids])


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [0, 2])
@pytest.mark.parametrize('k', KS)
def test_both_code_layouts_equal_the_oracle(world, index, k, variant):
    index.nprobe = NLIST
    index.set_scan_variant(variant)
    Dg, Ig = index.search(world['xq'], k)
    assert index.codes_mmajor or variant == 2     # the default path did scan the sub-quantiser-major copy
    Do, Io = world['rows'][k]
    assert np.array_equal(Ig, Io), np.nonzero((Ig != Io).any(1))[0]
    assert np.array_equal(_bits(Dg), _bits(Do)), np.nonzero((_bits(Dg) != _bits(Do)).any(1))[0]


@pytest.mark.gpu
@pytest.mark.parametrize('k', KS)
def test_the_window_scan_with_an_open_window_equals_the_oracle(world, index, k):
    """The RANGED instantiation over the window-ordered layout (every list sorted by the key: other tile
    positions for the same vectors); the window passes everything."""
    rng = np.random.default_rng(5)
    key = (300.0 + 600.0 * rng.random(N)).astype(np.float32)
    q_pmz = np.full(NQ, 600.0, np.float64)
    index.nprobe = NLIST
    index.set_scan_variant(0)
    index.set_window_key(key)
    Dg, Ig = index.search_window(world['xq'], k, q_pmz, 2, 1e9, 'Da')
    Do, Io = world['rows'][k]
    assert np.array_equal(Ig, Io), np.nonzero((Ig != Io).any(1))[0]
    assert np.array_equal(_bits(Dg), _bits(Do))


@pytest.mark.gpu
def test_rank_of_agrees_with_the_position_in_the_rows(world, index):
    Do, Io = world['rows'][512]
    for shift in (0, 131, 259, 260, 452):     # among them the constant rows' neighbours and the one-vector list
        T = ((np.arange(NQ) * 57 + shift) % N).astype(np.int64)
        rank, score, scope = index.rank_of(world['xq'], T, 0)
        want = np.array([int(np.nonzero(Io[i] == T[i])[0][0]) for i in range(NQ)])
        assert np.array_equal(rank, want), (shift, rank, want)
        assert (scope == N).all()
        assert np.array_equal(_bits(score), _bits(Do[np.arange(NQ), want]))
