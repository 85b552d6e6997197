"""IVF-PQ on the raw vectors (FAISS' ``IndexIVFPQ::by_residual = false``) against the oracle: training,
encoding, every scan path, the window scan, the rank scan, the exact re-rank, shards, persistence, the
state rules and the engine. The reference is the untouched oracle driven by tests/raw_pq_ref.py (a
one-row table of zeros for a centroid, ``adc(lut, code, 0.0)`` for a score). Data, sizes and seeds are
those of test_gpu_pq_shapes.py; everything is compared as integers / uint32 bits, no tolerance, ties
included."""
import struct

import numpy as np
import pytest

import raw_pq_ref as R
from test_gpu_pq_shapes import NITER, NLIST, SEED, _dense, _hashed

pytestmark = pytest.mark.gpu

ids_of = lambda s: 'd%d-m%d-b%d' % s
TRAIN = [(800, 32, 8), (800, 16, 4), (128, 4, 8), (132, 4, 8)]          # (800, 16, 4): subsampled training; dsub 32 / 33
ENCODE = [(800, 32, 8), (800, 16, 8), (800, 8, 8), (132, 4, 8)]          # register | one piece (dsub 50) | rounds | dsub 33
TILED = (800, 32, 8)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope='module')
def world(O):
    """shape -> the oracle's side of a raw-code index, computed once: vectors, coarse centroids, list
    assignment, the raw quantiser and codes, the inverted lists."""
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
            cb, codes = R.raw_quantiser(O, xb, m, 1 << bits, NITER, SEED + 7)
            full[shape] = dict(xb=xb, xq=xq, cen=cen, cb=cb, assign=a, codes=codes, ivf=O.HostIVF(cen, a, codes, cb))
        return full[shape]
    return get


def _new_index(shape, raw=True, nlist=NLIST):
    from ann_solo_amd import faiss_compat as faiss
    d, m, bits = shape
    idx = faiss.IndexIVFPQ(faiss.IndexFlatIP(d), d, nlist, m, bits)
    assert idx.by_residual is True                 # the default
    if raw:
        idx.by_residual = False
        assert idx.by_residual is False
    return idx


@pytest.fixture(scope='module')
def filled():
    """shape -> a raw-code index holding the oracle's quantisers and the library (one per shape)."""
    made = {}

    def get(shape, w):
        if shape not in made:
            idx = _new_index(shape)
            idx.set_trained(w['cen'], w['cb'])
            idx.add(w['xb'])
            made[shape] = idx
        return made[shape]
    return get


def _assert_rows(got, want, what):
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(_bits(got[0]), _bits(want[0])), what


# ---------------------------------------------------------------- 1. training
@pytest.mark.parametrize('shape', TRAIN, ids=ids_of)
def test_train_bit_exact(world, shape):
    d, m, bits = shape
    w = world(shape)
    xb = w['xb']
    if shape == (800, 16, 4):
        assert len(xb) > (1 << bits) * 256         # pq_train_device takes the permutation subsample
    both = {}
    for raw in (True, False):
        idx = _new_index(shape, raw)
        idx.set_niter(NITER)
        idx.seed = SEED
        idx.train(xb)
        assert idx.is_trained and idx.by_residual is (not raw)
        both[raw] = idx.centroids(), idx.codebooks()
    assert np.array_equal(_bits(both[True][0]), _bits(w['cen']))
    assert np.array_equal(_bits(both[True][0]), _bits(both[False][0]))        # the lists do not depend on the mode
    assert np.array_equal(_bits(both[True][1]), _bits(w['cb']))
    assert not np.array_equal(_bits(both[True][1]), _bits(both[False][1]))    # the quantiser does


# ---------------------------------------------------------------- 2. encoding
@pytest.mark.parametrize('shape', ENCODE, ids=ids_of)
def test_encode_and_lists_bit_exact(O, world, shape):
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
    # the same quantiser installed in a by-residual index codes x - centroid: other codes, same lists
    res = _new_index(shape, raw=False)
    res.set_trained(w['cen'], w['cb'])
    res.add(xb)
    off2, ids2, codes2 = res.lists()
    assert np.array_equal(off2, off) and np.array_equal(ids2, ids)
    assert np.array_equal(codes2, O.HostIVF(w['cen'], w['assign'], O.pq_encode(xb, w['cen'], w['assign'], w['cb']),
                                            w['cb']).payload)
    assert not np.array_equal(codes2, codes)


@pytest.mark.parametrize('shape', [(800, 8, 8), (132, 4, 8), (128, 4, 8)], ids=ids_of)
def test_encode_with_identical_codes_takes_the_lowest(O, world, shape):
    """Several codes that are the same point: the code is the lowest of them (rounds, one-piece and register path)."""
    w = world(shape)
    cb = w['cb'].copy()
    ksub = cb.shape[1]
    cb[:, ksub - 1] = cb[:, 3]
    cb[:, ksub // 2] = cb[:, 3]
    cb[:, 9] = cb[:, 200]
    idx = _new_index(shape)
    idx.set_trained(w['cen'], cb)
    idx.add(w['xb'])
    want = R.raw_codes(O, w['xb'], cb)
    assert (want == 3).any() and (want == 9).any()
    assert not (want == ksub - 1).any() and not (want == ksub // 2).any() and not (want == 200).any()
    ivf = O.HostIVF(w['cen'], w['assign'], want, cb)
    off, ids, codes = idx.lists()
    assert np.array_equal(ids, ivf.ids)
    assert np.array_equal(codes, ivf.payload)


# ---------------------------------------------------------------- 3. search
def test_search_tiled_identical_to_the_reference_and_unlike_by_residual(O, world, filled):
    w = world(TILED)
    idx, ivf, xq = filled(TILED, w), w['ivf'], w['xq']
    res = _new_index(TILED, raw=False)             # the same data, quantised by residual (its own quantiser)
    res.set_niter(NITER)
    res.seed = SEED
    res.train(w['xb'])
    assert np.array_equal(_bits(res.centroids()), _bits(w['cen']))
    res.add(w['xb'])
    for k, nprobe in ((64, 8), (1024, 8), (64, 16), (1024, 16)):
        idx.nprobe = res.nprobe = nprobe
        got = idx.search(xq, k)
        want = R.raw_search(O, xq, w['cen'], ivf, k, nprobe)
        _assert_rows(got, want, (k, nprobe))
        # coarse() is the real q . centroid in either mode
        cD, cI = idx.coarse(xq, nprobe)
        oD, oI = O.coarse(xq, w['cen'], nprobe)
        assert np.array_equal(cI, oI) and np.array_equal(_bits(cD), _bits(oD))
        # the tie rows, in the oracle's order: an all-zero query scores every vector 0.0, ascending ids
        for z in (5, 77, 199):
            v = want[1][z] >= 0
            assert (want[0][z][v] == 0.0).all() and (np.diff(want[1][z][v]) > 0).all()
        if k == 1024 and nprobe == 16:             # the copy of library row 7: its 51 equal codes, ascending ids
            at = int(np.nonzero(want[1][11] == 7)[0][0])
            assert want[1][11][at:at + 51].tolist() == [7] + list(range(4900, 4950))
            assert len(set(_bits(want[0][11][at:at + 51]).tolist())) == 1
        # and the by-residual index over the same vectors answers other rows, for every query that is not all zero
        Dr, Ir = res.search(xq, k)
        # (an all-zero query scores every vector 0.0 in both)
        differs = [(not np.array_equal(Ir[i], got[1][i])) or (not np.array_equal(_bits(Dr[i]), _bits(got[0][i])))
                   for i in range(len(xq)) if i not in (5, 77, 199)]
        assert all(differs), (k, nprobe, int(np.sum(differs)))


@pytest.mark.parametrize('shape', [(992, 32, 8), (1024, 32, 8)], ids=ids_of)
def test_search_on_both_sides_of_the_tiled_limit(O, shape):
    from ann_solo_amd import _lib
    d, m, bits = shape
    rng = np.random.default_rng(d)
    xb = rng.standard_normal((1500, d)).astype(np.float32)
    xb[1400:1450] = xb[3]
    xq = rng.standard_normal((40, d)).astype(np.float32)
    xq[2] = 0.0
    xq[5] = xb[3]
    cen = O.kmeans(xb, 4, 1, SEED, 0, 256)
    a = O.assign(xb, cen, 0)
    cb, codes = R.raw_quantiser(O, xb, m, 256, 1, SEED + 7)
    ivf = O.HostIVF(cen, a, codes, cb)
    idx = _new_index(shape, nlist=4)
    idx.set_niter(1)
    idx.seed = SEED
    idx.train(xb)
    assert np.array_equal(_bits(idx.centroids()), _bits(cen))
    assert np.array_equal(_bits(idx.codebooks()), _bits(cb))
    idx.add(xb)
    off, ids, got_codes = idx.lists()
    assert np.array_equal(off, ivf.list_offsets) and np.array_equal(ids, ivf.ids)
    assert np.array_equal(got_codes, ivf.payload)
    assert _lib.lib().asl_index_supports_keys(idx._h, 200, 2) == int(d <= 1020)     # the tiled scan is / is not in use
    for k, nprobe in ((1, 1), (200, 2), (1024, 4), (1024, 1)):
        idx.nprobe = nprobe
        _assert_rows(idx.search(xq, k), R.raw_search(O, xq, cen, ivf, k, nprobe), (k, nprobe))


@pytest.mark.parametrize('shape', [(800, 16, 8), (800, 32, 5)], ids=ids_of)
def test_search_generic_identical_to_the_reference(O, world, filled, shape):
    w = world(shape)
    idx, ivf, xq = filled(shape, w), w['ivf'], w['xq']
    grid = [(1, 1), (200, 8), (1024, 16), (1024, 1)]
    if shape == (800, 16, 8):
        grid.append((4096, 16))                    # k beyond TK_MAX_K: the bounded passes
    for k, nprobe in grid:
        idx.nprobe = nprobe
        _assert_rows(idx.search(xq, k), R.raw_search(O, xq, w['cen'], ivf, k, nprobe), (k, nprobe))


# ---------------------------------------------------------------- 4. the caller's coarse scores
def test_search_preassigned_ignores_coarse_scores_in_raw_mode(O, world, filled):
    w = world(TILED)
    idx, xq = filled(TILED, w), w['xq']
    cD, cI = idx.coarse(xq, 8)
    wrong = np.ascontiguousarray(cD[:, ::-1] * np.float32(3.0) + np.float32(1.25))
    want = R.raw_search(O, xq, w['cen'], w['ivf'], 200, 8)
    _assert_rows(idx.search_preassigned(xq, 200, cD, cI), want, 'right coarse_D')
    _assert_rows(idx.search_preassigned(xq, 200, wrong, cI), want, 'wrong coarse_D')
    res = _new_index(TILED, raw=False)
    res.set_trained(w['cen'], w['cb'])
    res.add(w['xb'])
    Da, Ia = res.search_preassigned(xq, 200, cD, cI)
    Db, Ib = res.search_preassigned(xq, 200, wrong, cI)
    assert not np.array_equal(_bits(Da), _bits(Db))


# ---------------------------------------------------------------- 5. window scan
def _window_mask(q_pmz, key, charge, tol, mode):
    l = np.asarray(key, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        if mode == 'Da':
            return np.abs(q_pmz - l) * float(charge) <= tol
        return np.abs(q_pmz - l) / l * 1000000.0 <= tol


def test_window_scan_identical_to_the_masked_reference(O, world, filled):
    w = world(TILED)
    idx, ivf, xq = filled(TILED, w), w['ivf'], w['xq'][:48]
    rng = np.random.default_rng(17)
    key0 = rng.uniform(400.0, 1400.0, len(w['xb'])).astype(np.float32)
    key_nan = key0.copy()
    key_nan[::7] = np.nan
    q_pmz = rng.uniform(500.0, 1300.0, len(xq))
    idx.nprobe = 8
    short = 0
    for key, tol, mode, k in ((key0, 250.0, 'Da', 256), (key0, 2.0, 'Da', 64), (key_nan, 300.0, 'Da', 200)):
        idx.set_window_key(key)
        D, I = idx.search_window(xq, k, q_pmz, 2, tol, mode)
        keep = np.stack([_window_mask(q_pmz[i], key, 2, tol, mode) for i in range(len(xq))])
        for i in range(0, len(xq), 9):             # the vectorised window test is the oracle's precursor_ok
            for j in range(0, 5000, 499):
                assert bool(keep[i, j]) == O.precursor_ok(q_pmz[i], key[j], 2, tol, mode)
        rD, rI = R.raw_search(O, xq, w['cen'], ivf, k, 8, keep=keep)
        assert np.array_equal(I, rI), (tol, mode, k)
        v = rI >= 0
        assert np.array_equal(_bits(D)[v], _bits(rD)[v]), (tol, mode, k)
        short += int((~v).any())
    assert short > 0


# ---------------------------------------------------------------- 6. rank
@pytest.mark.parametrize('nprobe', [8, 0], ids=['probed', 'exhaustive'])
def test_rank_of_agrees_with_the_search_rows(O, world, filled, nprobe):
    w = world(TILED)
    idx, xq = filled(TILED, w), w['xq'][:32]
    scan_probe = nprobe if nprobe else NLIST
    refD, refI = R.raw_search(O, xq, w['cen'], w['ivf'], 1024, scan_probe)
    valid = (refI >= 0).sum(1)
    target = np.array([refI[i, (i * 37) % max(1, valid[i])] for i in range(32)], np.int64)
    _, cI = O.coarse(xq, w['cen'], scan_probe)
    if nprobe:                                     # two targets outside the probed lists: not in scope
        for i in (3, 20):
            target[i] = int(np.nonzero(~np.isin(w['assign'], cI[i]))[0][0])
    rank, score, scope = idx.rank_of(xq, target, nprobe=nprobe)
    idx.nprobe = scan_probe
    D, I = idx.search(xq, 1024)
    in_scope = 0
    for i in range(32):
        if nprobe and i in (3, 20):
            assert rank[i] == -1 and np.isnan(score[i])
            assert target[i] not in I[i]
            continue
        r = int(rank[i])
        assert 0 <= r < 1024 and I[i, r] == target[i] and target[i] not in I[i, :r]
        assert _bits(score[i:i + 1])[0] == _bits(D[i, r:r + 1])[0] == _bits(refD[i, r:r + 1])[0]
        # the search's row holds the target for k = rank + 1 and not for k = rank
        _, Ik = idx.search(xq[i:i + 1], r + 1)
        assert Ik[0, r] == target[i]
        if r:
            _, Ik = idx.search(xq[i:i + 1], r)
            assert target[i] not in Ik[0]
        in_scope += 1
    assert in_scope >= 30
    sizes = np.diff(w['ivf'].list_offsets)
    assert np.array_equal(scope, sizes[cI].sum(1) if nprobe else np.full(32, len(w['xb'])))


# ---------------------------------------------------------------- 7. exact re-rank
def test_refine_over_the_raw_short_list(O, world):
    w = world(TILED)
    xb, xq, k = w['xb'], w['xq'], 100
    idx = _new_index(TILED)
    idx.set_refine(2 * k)                           # before add(): the exact rows are stored as vectors arrive
    idx.set_trained(w['cen'], w['cb'])
    idx.add(xb)
    for nprobe in (1, 8):
        idx.nprobe = nprobe
        _, I_short = R.raw_search(O, xq, w['cen'], w['ivf'], 2 * k, nprobe)
        _assert_rows(idx.search(xq, k), O.refine(xb, xq, I_short, k), nprobe)


# ---------------------------------------------------------------- 8. shards
def test_three_shards_merge_to_the_unsharded_rows(O, world, filled):
    from ann_solo_amd import faiss_compat as faiss
    w = world(TILED)
    full, xq = filled(TILED, w), w['xq']
    full.nprobe = 8
    D, I = full.search(xq, 1024)
    _assert_rows((D, I), R.raw_search(O, xq, w['cen'], w['ivf'], 1024, 8), 'unsharded')
    parts = []
    for r in range(3):
        sh = _new_index(TILED)
        sh.set_trained(w['cen'], w['cb'])
        sh.add(w['xb'])
        sh.shard(r, 3)
        assert sh.by_residual is False
        assert sh.ntotal == len(w['xb']) and sh.info().nlocal < len(w['xb'])
        sh.nprobe = 8
        parts.append(sh.search(xq, 1024))
    Dm, Im = faiss.topk_merge(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]))
    assert np.array_equal(Im, I) and np.array_equal(_bits(Dm), _bits(D))


# ---------------------------------------------------------------- 9. persistence
def test_save_and_load(O, world, filled, tmp_path):
    from ann_solo_amd import faiss_compat as faiss
    from ann_solo_amd._lib import AnnSoloMiError
    w = world(TILED)
    idx, xq = filled(TILED, w), w['xq']
    idx.nprobe = 8
    D, I = idx.search(xq, 200)
    raw_path = str(tmp_path / 'raw.idxmi')
    faiss.write_index(idx, raw_path)
    blob = open(raw_path, 'rb').read()
    version, pad = struct.unpack_from('<i', blob, 8)[0], struct.unpack_from('<i', blob, 68)[0]
    assert version == 3 and pad == 1 << 30          # header: magic[8], 8 int32, 2 int64, 4 int32 (pad last)
    back = faiss.read_index(raw_path)
    assert back.by_residual is False and back.is_trained and back.ntotal == len(w['xb'])
    assert np.array_equal(_bits(back.codebooks()), _bits(w['cb']))
    assert np.array_equal(back.lists()[2], idx.lists()[2])
    back.nprobe = 8
    _assert_rows(back.search(xq, 200), (D, I), 'loaded raw index')
    with pytest.raises(AnnSoloMiError):             # the mode is the file's
        back.by_residual = True
    # raw codes with exact rows: the refine bits stay where they were
    ref = _new_index(TILED)
    ref.set_refine(200)
    ref.set_trained(w['cen'], w['cb'])
    ref.add(w['xb'][:500])
    p2 = str(tmp_path / 'raw_refine.idxmi')
    faiss.write_index(ref, p2)
    assert struct.unpack_from('<i', open(p2, 'rb').read(), 68)[0] == (1 << 30) | 1 | (200 << 1)
    b2 = faiss.read_index(p2)
    assert b2.by_residual is False and b2.refine_k == 200
    # a by-residual index: byte for byte the file of an index that never heard of the switch
    files = []
    for touch in (False, True):
        r = _new_index(TILED, raw=False)
        if touch:
            r.by_residual = False
            r.by_residual = True
        r.set_trained(w['cen'], w['cb'])
        r.add(w['xb'][:1000])
        p = str(tmp_path / ('res%d.idxmi' % touch))
        faiss.write_index(r, p)
        files.append(open(p, 'rb').read())
    assert files[0] == files[1]
    assert struct.unpack_from('<i', files[0], 8)[0] == 2 and struct.unpack_from('<i', files[0], 68)[0] == 0
    assert faiss.read_index(str(tmp_path / 'res0.idxmi')).by_residual is True
    # the bit in a version-2 header, and a version-3 header with the bit on an IVF-Flat kind, are refused
    bad = bytearray(blob)
    bad[8:12] = struct.pack('<i', 2)
    p = str(tmp_path / 'bit_in_v2.idxmi')
    open(p, 'wb').write(bytes(bad))
    with pytest.raises(AnnSoloMiError) as e:
        faiss.read_index(p)
    assert 'bad refine / storage fields' in str(e.value)
    flat = faiss.IndexIVFFlat(faiss.IndexFlatIP(800), 800, NLIST)
    flat.set_trained(w['cen'])
    flat.add(w['xb'][:300])
    p = str(tmp_path / 'flat.idxmi')
    faiss.write_index(flat, p)
    fb = bytearray(open(p, 'rb').read())
    assert faiss.read_index(p).by_residual is True
    fb[8:12] = struct.pack('<i', 3)
    fb[68:72] = struct.pack('<i', struct.unpack_from('<i', fb, 68)[0] | (1 << 30))
    open(p, 'wb').write(bytes(fb))
    with pytest.raises(AnnSoloMiError) as e:
        faiss.read_index(p)
    assert 'bad refine / storage fields' in str(e.value)
    # a truncated raw file still fails the exact size check
    p = str(tmp_path / 'short.idxmi')
    open(p, 'wb').write(blob[:-1])
    with pytest.raises(AnnSoloMiError) as e:
        faiss.read_index(p)
    assert 'file size' in str(e.value)


# ---------------------------------------------------------------- 10. state rules
def test_state_errors(O, world):
    from ann_solo_amd import _lib, faiss_compat as faiss
    from ann_solo_amd._lib import AnnSoloMiError
    L = _lib.lib()
    ASL_ERR_STATE, ASL_ERR_INVALID = -3, -1
    w = world(TILED)
    flat = faiss.IndexIVFFlat(faiss.IndexFlatIP(800), 800, NLIST)
    assert L.asl_index_set_by_residual(flat._h, 0) == ASL_ERR_STATE
    assert b'IVF-PQ' in L.asl_last_error()
    assert L.asl_index_set_by_residual(flat._h, 1) == ASL_ERR_STATE
    assert flat.by_residual is True
    plain = faiss.IndexFlatIP(800)
    assert L.asl_index_set_by_residual(plain._h, 0) == ASL_ERR_STATE and plain.by_residual is True
    idx = _new_index(TILED, raw=False)
    assert L.asl_index_set_by_residual(idx._h, 2) == ASL_ERR_INVALID
    idx.set_trained(w['cen'], w['cb'])
    assert L.asl_index_set_by_residual(idx._h, 0) == ASL_ERR_STATE      # after set_trained
    with pytest.raises(AnnSoloMiError):
        idx.by_residual = False
    assert idx.by_residual is True
    small = _new_index((128, 4, 8))
    xs = world((128, 4, 8))['xb']
    small.set_niter(1)
    small.train(xs)
    with pytest.raises(AnnSoloMiError):                                # after train
        small.by_residual = True
    assert small.by_residual is False
    # set_trained after by_residual = False, then add: raw codes -- and the flag outlives reset()
    raw = _new_index(TILED)
    raw.set_trained(w['cen'], w['cb'])
    raw.add(w['xb'])
    assert np.array_equal(raw.lists()[2], w['ivf'].payload)
    raw.reset()
    assert raw.by_residual is False and raw.ntotal == 0
    raw.add(w['xb'][:2000])
    keep = w['ivf'].ids < 2000
    assert np.array_equal(raw.lists()[2], w['ivf'].payload[keep])


# ---------------------------------------------------------------- 11. the engine
def _engine_reference(O, sl, q, k, nprobe, tol, mode, niter, seed, pre):
    part = sl.partitions[2]
    Ls = O.Spectra(*part.spectra.to('cpu').numpy())
    Qs = O.Spectra(*q.numpy())
    xb = O.encode_batch(Ls.mz, Ls.intensity, Ls.offsets, 10.96, 0.04, 800)
    xq = O.encode_batch(Qs.mz, Qs.intensity, Qs.offsets, 10.96, 0.04, 800)
    cen = O.kmeans(xb, NLIST, niter, seed, 0, 256)
    a = O.assign(xb, cen, 0)
    cb, codes = R.raw_quantiser(O, xb, 32, 256, niter, seed + 7)
    ivf = O.HostIVF(cen, a, codes, cb)
    key = np.ascontiguousarray(part.precursor_mz, np.float32)
    keep = np.stack([_window_mask(Qs.precursor_mz[i], key, 2, tol, mode) for i in range(Qs.n)])
    out = dict(cen=cen, cb=cb, ivf=ivf)
    for name, mask in (('post', None), ('pre', keep)) if pre else (('post', None),):
        _, knn = R.raw_search(O, xq, cen, ivf, k, nprobe, keep=mask)
        best_row, best_score = np.empty(Qs.n, np.int32), np.empty(Qs.n, np.float64)
        n_cand, pm = np.empty(Qs.n, np.int32), []
        for i in range(Qs.n):
            cand = np.sort(np.array([r for r in knn[i] if r >= 0 and O.precursor_ok(Qs.precursor_mz[i], key[r], 2, tol, mode)],
                                    np.int64))
            b, sc, pairs = O.best_match(Qs, i, Ls, cand, 0.02, True) if len(cand) else (-1, 0.0, np.zeros((0, 2), np.uint32))
            n_cand[i] = len(cand)
            best_row[i] = cand[b] if b >= 0 else -1
            best_score[i] = sc if b >= 0 else 0.0
            pm.append(pairs if b >= 0 else pairs[:0])
        out[name] = dict(knn=knn, best_row=best_row, best_score=best_score, n_cand=n_cand, pm=pm)
    return out


def _assert_engine(res, ref, what, knn=True):
    g = lambda a: a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)
    if knn:
        assert np.array_equal(g(res.knn), ref['knn']), what
    assert np.array_equal(g(res.best_row), ref['best_row']), what
    assert np.array_equal(g(res.best_score), ref['best_score']), what
    assert np.array_equal(g(res.n_candidates), ref['n_cand']), what
    cnt, pairs = g(res.pm_count), g(res.pm_pairs)
    for i, want in enumerate(ref['pm']):
        assert cnt[i] == len(want), (what, i)
        n = min(len(want), pairs.shape[1])
        assert np.array_equal(pairs[i, :n], want[:n]), (what, i)


def test_engine_end_to_end_and_cache_of_the_other_mode(O, tmp_path, caplog):
    import logging
    import os
    import shutil
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    from test_gpu_window_scan import _queries, _tie_library
    lib0, aux, lib = _tie_library()
    q = _queries(lib0, aux, 64, seed=72, with_copies=8)
    base = dict(index='ivfpq', num_list=16, num_probe=8, num_candidates=256, kmeans_niter=4)
    ref = None
    for window in ('post', 'pre'):
        cfg = Config.open_search(pq_by_residual=False, ann_window=window, **base)
        (tmp_path / window).mkdir()
        sl = SpectralLibrary(lib, config=cfg, index_dir=str(tmp_path / window), basename='lib')
        try:
            if ref is None:
                ref = _engine_reference(O, sl, q, 256, 8, 300.0, 'Da', 4, 1234, pre=True)
                assert (ref['post']['best_row'] >= 0).mean() > 0.5
                assert not np.array_equal(ref['post']['knn'], ref['pre']['knn'])
            idx = sl._get_ann_index(2)
            assert idx.by_residual is False
            assert np.array_equal(_bits(idx.centroids()), _bits(ref['cen']))
            assert np.array_equal(_bits(idx.codebooks()), _bits(ref['cb']))
            assert np.array_equal(idx.lists()[2], ref['ivf'].payload)
            _assert_engine(sl._search_batch(q, 2, 'open', want_knn=True), ref[window], (window, 'sync knn'))
            _assert_engine(sl._search_batch(q, 2, 'open'), ref[window], (window, 'sync'), knn=False)
            sl.set_pipeline(True)
            try:
                qd = q.to('cuda:0')
                a_ = sl._search_batch(qd, 2, 'open', device_out=True)
                b_ = sl._search_batch(qd, 2, 'open', device_out=True, want_knn=True)
                sl.synchronize()
            finally:
                sl.set_pipeline(False)
            _assert_engine(a_, ref[window], (window, 'pipelined'), knn=False)
            _assert_engine(b_, ref[window], (window, 'pipelined knn'))
            raw_file = sl._ann_filenames[2]
        finally:
            sl.shutdown()
    # a cached file of the other mode under this configuration's name is rebuilt, not searched
    (tmp_path / 'res').mkdir()
    other = SpectralLibrary(lib, config=Config.open_search(**base), index_dir=str(tmp_path / 'res'), basename='lib')
    try:
        assert other._get_ann_index(2).by_residual is True
        res_file = other._ann_filenames[2]
        by_res = other._search_batch(q, 2, 'open', want_knn=True)
        assert not np.array_equal(by_res.knn, ref['post']['knn'])
    finally:
        other.shutdown()
    assert os.path.basename(res_file) != os.path.basename(raw_file)      # the hash in the name tells the modes apart
    shutil.copyfile(res_file, raw_file)
    cfg = Config.open_search(pq_by_residual=False, ann_window='pre', **base)
    with caplog.at_level(logging.WARNING):
        again = SpectralLibrary(lib, config=cfg, index_dir=str(tmp_path / 'pre'), basename='lib')
        try:
            idx = again._get_ann_index(2)
            assert idx.by_residual is False
            assert any('does not match' in r.getMessage() for r in caplog.records)
            _assert_engine(again._search_batch(q, 2, 'open', want_knn=True), ref['pre'], 'rebuilt')
        finally:
            again.shutdown()
