"""The control flow of the tiled IVF-PQ scan's tile loop, at the places where a wave leaves its hot loop.

The loop scores a tile, ballots the lanes that pass the threshold snapshot and falls through one scalar test
(no passer, flag down, no exact flushes); everything else -- the reservation, a refused reservation and its retry
behind the sync, a sync another wave asked for, the exact-flush test -- runs off that path, and the rotation of the
two register sets is walked to its end there before the hot loop starts over at set 0. What that can break and the
other files do not pin at every position:

  * a refused reservation at both rotation positions of every wave: a list of 3 000 copies of ONE vector (more
    equal scores than the 2 048-key buffer holds: refused reservations, then exact flushes) whose first tile is
    table entry t, t = 0..15 -- entry i of wave w is its tile number (i - w) / 8, so 16 placements put the first
    refusal at both sets of all 8 waves -- with further lists behind it and, the same placements, as the LAST
    list probed, so that the waves that finish their share first join the syncs from the wait;
  * a sync asked for by one wave while the tiles of the others hold no passer: every list is one tile, table
    entry r is the list of probe rank r, and only the entries r = w (mod 8), wave w's, hold near neighbours (4 096
    of them, scores rising with r, k = 64), for w = 0 and w = 7;
  * the early outs: a query for which no tile behind the first chunk of 256 entries has a passer (the first sync,
    inside that chunk, lifts the threshold above every later score), and one for which every lane of every tile
    passes until the buffer is full (the copies, k = 1 024);
  * the threshold's edge: scores equal to the threshold (the copies: ties pass `>=`), the all-zero query (every
    score is its list's coarse term, +0.0) and a query whose scores are negative, on the ordered-key path;
  * every shape once: k = 1 024 and 1 500, tables of 255 / 256 / 257 / 513 entries, two probes per thread (600
    lists), the window scan at 167 / 168 / 169 entries, the selected scan at 256 / 257, set-mode rows with the
    scan-side precursor filter.

d = 800, m = 32, 8 bits, 512 lists filled through asl_index_add_preassigned, nprobe = nlist: the table of a query
is the whole index in ITS probe order, which the oracle's coarse search gives. The default scan
(sub-quantiser-major) and variant 2 (tile-major) against each other and against the oracle: ids and score bits
equal, no tolerance."""
import numpy as np
import pytest

import interval_ref as IR
import selector_ref as SR
from test_gpu_pq_prefetch import _bits, _index, _window_entries

pytestmark = pytest.mark.gpu

D, M, NLIST, SEED = 800, 32, 512, 9173
DUP_N = 3000
N_LIB = 10000
Q_DUP, Q_NEG, Q_ZERO, Q_REG = 0, 1, 2, 3        # rows of a case's query block; regular queries from Q_REG on
N_REG = 5


@pytest.fixture(scope='module')
def base(O):
    from ann_solo_amd import synthetic
    rng = np.random.default_rng(SEED)
    lib, aux = synthetic.make_library(N_LIB, seed=611, device='cpu')
    q, _ = synthetic.make_queries(lib, aux, 40, seed=612)
    o, mz, inten, *_ = lib.numpy()
    xb = O.encode_batch(mz, inten, o, 10.96, 0.04, D)
    o, mz, inten, *_ = q.numpy()
    xq = O.encode_batch(mz, inten, o, 10.96, 0.04, D)
    cen = np.ascontiguousarray(xb[rng.choice(N_LIB, NLIST, replace=False)])
    cb = O.pq_train(xb[:4000], cen, M, 256, 2, SEED + 7)
    return dict(xb=xb, xq=xq, cen=cen, cb=cb, rng=rng)


def _probe_order(O, cen, qv):
    """List ids in the order the query probes them (the order of its tile table)."""
    return O.coarse(np.ascontiguousarray(qv[None], np.float32), cen, len(cen))[1][0]


def _assign_by_rank(order, sizes_by_rank, nlist=NLIST):
    """assign[i] for sum(sizes) vectors: the first sizes[0] go to the list of probe rank 0, and so on."""
    sizes = np.zeros(nlist, np.int64)
    sizes[:len(sizes_by_rank)] = sizes_by_rank
    return np.repeat(order.astype(np.int32), sizes)


def _both_layouts_and_oracle(O, base, x, assign, xq, ks, nlist=NLIST, cen=None):
    cen = base['cen'] if cen is None else cen
    ivf = O.HostIVF(cen, assign, O.pq_encode(x, cen, assign, base['cb']), base['cb'])
    idx = _index(cen, base['cb'], x, assign, nlist)
    out = {}
    for k in ks:
        Do, Io = ivf.search(xq, k, nlist)
        idx.set_scan_variant(2)
        Dt, It = idx.search(xq, k)
        idx.set_scan_variant(0)
        Dm, Im = idx.search(xq, k)
        assert idx.codes_mmajor
        assert np.array_equal(Im, It) and np.array_equal(_bits(Dm), _bits(Dt)), k
        assert np.array_equal(Im, Io) and np.array_equal(_bits(Dm), _bits(Do)), k
        out[k] = (Do, Io)
    return out, ivf, idx


@pytest.mark.parametrize('t', range(16))
def test_refused_reservation_with_the_first_tile_of_the_copies_at_every_entry(O, base, t):
    xdup = base['xb'][7]
    order = _probe_order(O, base['cen'], xdup)
    fills = [1, 63, 64, 7, 33, 64, 2, 50]
    front = [fills[r % 8] for r in range(t)]               # t lists of one tile each in front of the copies
    for tail in ([40] * 20, []):                           # lists behind the copies / the copies probed last
        sizes = front + [DUP_N] + tail
        assign = _assign_by_rank(order, sizes)
        n = len(assign)
        x = base['xb'][100:100 + n].copy()
        dup_rows = np.arange(sum(front), sum(front) + DUP_N)
        x[dup_rows] = xdup
        tiles = (np.array(sizes) + 63) // 64
        assert tiles[:t].sum() == t and tiles[t] == 47     # the copies' first tile is table entry t
        xq = np.concatenate([xdup[None], -xdup[None], np.zeros((1, D), np.float32), base['xq'][:N_REG]])
        perm = np.random.default_rng(SEED + t).permutation(n)              # ids in no particular order
        res, _, _ = _both_layouts_and_oracle(O, base, x[perm], assign[perm], xq, (1024,))
        Do, Io = res[1024]
        dup_id = np.nonzero(np.isin(perm, dup_rows))[0]
        hit = np.isin(Io[Q_DUP], dup_id)
        # k cuts through the block of equal scores, which is larger than the key buffer: ties at the threshold
        assert hit[-1] and hit.sum() > 900 and len(np.unique(_bits(Do[Q_DUP][hit]))) == 1
        assert (Do[Q_NEG] < 0).sum() > 900                 # negative scores
        if not tail:                                       # ... down to the copies, the lowest of all: ordered keys
            neg = np.isin(Io[Q_NEG], dup_id)
            assert neg[-1] and neg.sum() > 500 and len(np.unique(_bits(Do[Q_NEG][neg]))) == 1
        assert (_bits(Do[Q_ZERO]) == 0).all()              # every score the coarse term +0.0


@pytest.mark.parametrize('w', [0, 7])
def test_sync_asked_for_by_one_wave_while_the_others_have_no_passer(O, base, w):
    rng = np.random.default_rng(SEED + 50 + w)
    qv = base['xq'][11]
    order = _probe_order(O, base['cen'], qv)
    near_rank = np.arange(NLIST) % 8 == w
    sizes = np.where(near_rank, 64, 12)
    assign = _assign_by_rank(order, sizes)
    n = len(assign)
    assert n <= 12000
    x = base['xb'][:n].copy()
    rank_of_row = np.repeat(np.arange(NLIST), sizes)
    # near neighbours: the query plus noise that shrinks with the probe rank, so later tiles score higher
    rows = np.nonzero(near_rank[rank_of_row])[0]
    noise = rng.standard_normal((len(rows), D)).astype(np.float32) / np.float32(np.sqrt(D))
    amp = (0.9 - 0.8 * rank_of_row[rows] / NLIST).astype(np.float32)[:, None]
    v = qv[None] + amp * noise
    x[rows] = v / np.linalg.norm(v, axis=1, keepdims=True).astype(np.float32)
    xq = np.concatenate([qv[None], base['xq'][:N_REG]])
    res, ivf, _ = _both_layouts_and_oracle(O, base, x, assign, xq, (64, 1024))
    Do, Io = res[64]
    assert near_rank[rank_of_row[Io[0]]].all()             # the 64 best are all in wave w's entries
    far = ~near_rank[rank_of_row]
    D_all, I_all = ivf.search(xq[:1], 4096 + 16, NLIST)
    n_near_first = int(np.argmax(far[I_all[0]]))           # near neighbours that beat every other vector
    assert n_near_first > 2048 + 64                        # more passers than the key buffer holds


def test_no_passer_behind_the_first_chunk(O, base):
    rng = np.random.default_rng(SEED + 90)
    qv = base['xq'][12]
    order = _probe_order(O, base['cen'], qv)
    sizes = [10] * 256 + [64] * 45                         # 2 560 vectors in the first chunk: a sync inside it
    assign = _assign_by_rank(order, sizes)
    n = len(assign)
    x = base['xb'][:n].copy()
    noise = rng.standard_normal((80, D)).astype(np.float32) / np.float32(np.sqrt(D))
    v = qv[None] + np.float32(0.3) * noise                 # ranks 0..7 hold 80 near neighbours
    x[:80] = v / np.linalg.norm(v, axis=1, keepdims=True).astype(np.float32)
    xq = np.concatenate([qv[None], base['xq'][:N_REG]])
    res, ivf, _ = _both_layouts_and_oracle(O, base, x, assign, xq, (64,))
    Dk, Ik = ivf.search(xq[:1], 128, NLIST)
    assert (Ik[0][:80] < 80).all() and (Ik[0][80:] >= 80).all()
    # the threshold bucket of the 64th best (0.0024 wide) lies above every other vector's score
    assert Dk[0][63] - Dk[0][80] > 0.01


@pytest.fixture(scope='module')
def lengths(O, base):
    made = {}

    def get(total, nlist=NLIST, cen=None):
        if (total, nlist) not in made:
            rng = np.random.default_rng(SEED + total + nlist)
            fills = rng.choice([1, 3, 7, 16, 63, 64], total - 1, p=[.4, .25, .2, .09, .03, .03])
            sizes = np.zeros(nlist, np.int64)
            sizes[:min(total - 1, nlist - 1)] = fills[:nlist - 1]
            left = total - int(((sizes + 63) // 64).sum())                 # the last list takes the rest
            sizes[min(total - 1, nlist - 1)] = 64 * (left - 1) + 5
            assert int(((sizes + 63) // 64).sum()) == total
            sizes = sizes[rng.permutation(nlist)]
            assign = rng.permutation(np.repeat(np.arange(nlist, dtype=np.int32), sizes))
            assert len(assign) <= N_LIB
            made[(total, nlist)] = (base['xb'][:len(assign)], assign)
        return made[(total, nlist)]
    return get


@pytest.mark.parametrize('total', [255, 256, 257, 513])
def test_table_lengths_around_a_chunk_with_both_key_buffers(O, base, lengths, total):
    x, assign = lengths(total)
    xq = np.concatenate([np.zeros((1, D), np.float32), base['xq'][:N_REG + 3]])
    _both_layouts_and_oracle(O, base, x, assign, xq, (1024, 1500))


def test_two_probes_per_thread(O, base, lengths):
    nlist = 600
    cen = np.ascontiguousarray(base['xb'][np.random.default_rng(SEED + 3).choice(N_LIB, nlist, replace=False)])
    x, assign = lengths(257, nlist)
    _both_layouts_and_oracle(O, base, x, assign, base['xq'][:N_REG + 3], (1024, 1500), nlist=nlist, cen=cen)


@pytest.mark.parametrize('total', [256, 257])
def test_selected_scan_around_a_chunk(O, base, lengths, total):
    x, assign = lengths(total)
    xq = base['xq'][:N_REG + 3]
    ivf = O.HostIVF(base['cen'], assign, O.pq_encode(x, base['cen'], assign, base['cb']), base['cb'])
    idx = _index(base['cen'], base['cb'], x, assign, NLIST)
    keep = np.arange(len(x)) % 3 != 1
    idx.set_selector(keep)
    try:
        for k in (64, 1024):
            got = idx.search_selected(xq, k)
            SR.assert_rows_equal(got, SR.search_selected(O, ivf, xq, k, NLIST, keep), k)
            hit = got[1][got[1] >= 0]
            assert keep[hit].all() and len(hit)
    finally:
        idx.set_selector(None)


def test_window_scan_around_its_chunk(O, base):
    w_nlist = 64
    sizes = np.array([168] * 54 + [100, 30, 200] + [0] * 7, np.int64)
    windows = ((5, 150), (40, 150), (5, 195), (40, 195))                   # ranks [a, b]
    assert [_window_entries(sizes, a, b) for a, b in windows] == [168, 167, 169, 168]
    n = int(sizes.sum())
    assign = np.random.default_rng(SEED + 1).permutation(np.repeat(np.arange(w_nlist, dtype=np.int32), sizes))
    cen = np.ascontiguousarray(base['cen'][:w_nlist])
    x = base['xb'][:n]
    ivf = O.HostIVF(cen, assign, O.pq_encode(x, cen, assign, base['cb']), base['cb'])
    key = np.empty(n, np.float32)                          # a vector's key: 500 + its rank in its list
    for l in range(w_nlist):
        ids = ivf.ids[ivf.list_offsets[l]:ivf.list_offsets[l + 1]]
        key[ids] = 500.0 + np.arange(len(ids), dtype=np.float32)
    xq = base['xq'][:8]
    wins = np.array([[500.0 + windows[i % 4][0] - 0.25, 500.0 + windows[i % 4][1] + 0.25] for i in range(len(xq))])
    idx = _index(cen, base['cb'], x, assign, w_nlist)
    idx.set_window_key(key)
    got = idx.search_window(xq, 1024, wins, 2, 0.0, 'interval')
    IR.assert_rows_equal(got, IR.index_rows(O, ivf, xq, 1024, w_nlist, key, wins))
    assert (got[1][:, 0] >= 0).all()


def test_set_mode_rows_with_the_scan_side_precursor_filter(O):
    from ann_solo_amd import _lib, synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, aux = synthetic.make_library(2000, seed=613, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, 64, seed=614, charge=2)
    cfg = Config.open_search(num_list=16, num_probe=6, num_candidates=128, index='ivfpq', kmeans_niter=3,
                             precursor_tolerance_mass_open=500, precursor_tolerance_mode_open='Da')
    prev = _lib.lib().asl_set_scan_postfilter(1)
    sl = SpectralLibrary(lib, config=cfg, device='cuda:0')
    try:
        part = sl.partitions[2]
        idx = sl._get_ann_index(2)
        info = idx.info()
        off, ids, codes = idx.lists()
        ivf = O.HostIVF.__new__(O.HostIVF)
        ivf.centroids, ivf.nlist, ivf.d = idx.centroids(), info.nlist, info.d
        ivf.list_offsets, ivf.ids, ivf.payload, ivf.codebooks, ivf.kind = off, ids, codes, idx.codebooks(), 1
        first = sl._search_batch(q, 2, 'open')
        ref = O.search_batch(O.Spectra(*q.numpy()), O.Spectra(*part.spectra.to('cpu').numpy()), part.precursor_mz,
                             2, ivf, 128, 6, 500, 'Da', 0.02, True, pm_stride=first.pm_pairs.shape[1])
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
