"""The tiled IVF-PQ scan's append of a tile that holds passers: the reservation, its verdict and the keys' places.

A tile with passers reserves its slots with one lane's add on the fill counter, settles the verdict (the reservation
ends at or below the buffer's capacity, or it is refused and nothing is written) as a scalar before the lanes part,
and every passing lane writes its key at base + the number of passers in the lanes below it (v_mbcnt on the scalar
mask), the score's ordered key made without a select. test_gpu_pq_tile_step.py pins refused reservations at every
position of the rotation; this file pins what the append itself can get wrong:

  * the lane's offset among the passers: behind a first list of 40 tiles (one sync: the threshold is finite) one-tile
    lists in which exactly chosen lanes hold near neighbours -- lane 0 only, lane 63 only, lanes 31 and 32 (the two
    halves of the mask), all even lanes, all 64 -- at k = 8, 64 and 1 024; a wrong offset overwrites or loses a key;
  * the verdict's edge: reservations that end exactly at the capacity (32 full tiles under the -inf threshold:
    accepted) and one past it (2 047 vectors, then a tile with 2 passers: refused, offered again behind the sync),
    with the 2 048-key and the 4 096-key buffer;
  * padding lanes: the only lists hold 1, 33 and 63 vectors and every lane "passes" the -inf threshold;
  * the empty-slot value: the all-zero query, whose best hit (score +0.0) is the vector of slot 0;
  * negative scores on the ordered-key path, the list of 3 000 copies taking the scan to exact flushes;
  * every kind of instantiation once: two probes per thread, the window scan, the selected scan, set-mode rows with
    the scan-side precursor filter; the tile-major layout runs beside the default one in every case.

d = 800, m = 32, 8 bits, 512 lists filled through asl_index_add_preassigned, nprobe = nlist (the cases of
test_gpu_pq_tile_step.py, whose helpers build them). The default scan and variant 2 against each other and against
the oracle: ids and score bits equal, no tolerance."""
import numpy as np
import pytest

import interval_ref as IR
import selector_ref as SR
from test_gpu_pq_prefetch import _bits, _index, _window_entries
from test_gpu_pq_tile_step import (D, NLIST, N_REG, SEED, DUP_N, _assign_by_rank, _both_layouts_and_oracle,
                                   _probe_order, base, lengths)  # noqa: F401  (base, lengths: fixtures)

pytestmark = pytest.mark.gpu

FIRST_TILES, N_PATTERN = 40, 24
PATTERNS = {'lane_0': [0], 'lane_63': [63], 'lanes_31_32': [31, 32], 'even_lanes': list(range(0, 64, 2)),
            'all_64': list(range(64))}


def _near(rng, qv, amp):
    """One unit vector per entry of amp: the query plus that much unit-length noise (cosine 1 / sqrt(1 + amp^2))."""
    amp = np.asarray(amp, np.float32).reshape(-1, 1)
    noise = rng.standard_normal((len(amp), D)).astype(np.float32) / np.float32(np.sqrt(D))
    v = qv[None] + amp * noise
    return v / np.linalg.norm(v, axis=1, keepdims=True).astype(np.float32)


def _stored_in_order(idx, l, rows):
    """List l holds exactly `rows`, in that order: lane v of its tile t is rows[64 * t + v]."""
    off, ids, _ = idx.lists()
    assert np.array_equal(ids[off[l]:off[l + 1]], rows)


@pytest.mark.parametrize('pattern', sorted(PATTERNS))
def test_the_lanes_offset_among_the_passers(O, base, pattern):
    lanes = np.array(PATTERNS[pattern])
    rng = np.random.default_rng(SEED + 300 + len(lanes) + int(lanes[0]))
    qv = base['xq'][13]
    order = _probe_order(O, base['cen'], qv)
    sizes = [64 * FIRST_TILES] + [64] * N_PATTERN
    assign = _assign_by_rank(order, sizes)
    n = len(assign)
    x = base['xb'][:n].copy()
    medium = np.arange(100)                                # in the first two tiles: they set the threshold
    x[medium] = _near(rng, qv, np.full(len(medium), 0.8))
    starts = 64 * FIRST_TILES + 64 * np.arange(N_PATTERN)
    near = (starts[:, None] + lanes[None]).ravel()         # the chosen lanes of every one-tile list
    amp = np.repeat(0.2 - 0.15 * np.arange(N_PATTERN) / N_PATTERN, len(lanes))     # later tiles score higher
    x[near] = _near(rng, qv, amp)
    xq = np.concatenate([qv[None], base['xq'][:N_REG]])
    res, ivf, idx = _both_layouts_and_oracle(O, base, x, assign, xq, (8, 64, 1024))
    for r in (1, N_PATTERN):
        _stored_in_order(idx, order[r], np.arange(starts[r - 1], starts[r - 1] + 64))
    # the construction, by the oracle's own (PQ) scores: the first 2 048 vectors scanned -- one sync -- hold the 100
    # medium neighbours, so the threshold of k = 8 and k = 64 is theirs; they and the chosen lanes lie a bucket
    # (0.0024) and more above every other vector, and every chosen lane passes the threshold of k = 64
    D_all, I_all = ivf.search(xq[:1], n, NLIST)
    score = np.empty(n, np.float32)
    score[I_all[0]] = D_all[0]
    rest = np.ones(n, bool)
    rest[medium] = rest[near] = False
    m64 = np.sort(score[medium])[-64]
    print('near %.4f..%.4f  medium %.4f..%.4f, 64th best %.4f  rest ..%.4f' % (
        score[near].min(), score[near].max(), score[medium].min(), score[medium].max(), m64, score[rest].max()))
    assert min(score[medium].min(), score[near].min()) > score[rest].max() + 0.01
    assert score[near].min() > m64
    for k in (8, 64):
        assert set(res[k][1][0]) <= set(near) | set(medium)
    if len(near) + len(medium) <= 1024:                    # every key of a chosen lane is among the k = 1 024 best
        assert set(near) <= set(res[1024][1][0])


@pytest.mark.parametrize('k,cap', [(1024, 2048), (1500, 4096)])
@pytest.mark.parametrize('past', [0, 1])
def test_a_reservation_that_ends_at_the_capacity_and_one_past_it(O, base, k, cap, past):
    order = _probe_order(O, base['cen'], base['xq'][0])
    # under the -inf threshold every stored vector passes: the fill level is the number of vectors scanned
    sizes = [64] * (cap // 64) if not past else [64] * (cap // 64 - 1) + [63, 2]
    assert sum(sizes) == cap + past
    assign = _assign_by_rank(order, sizes)
    x = base['xb'][200:200 + len(assign)]
    xq = np.concatenate([base['xq'][:N_REG], np.zeros((1, D), np.float32)])
    res, _, _ = _both_layouts_and_oracle(O, base, x, assign, xq, (k,))
    assert (res[k][1] >= 0).all()


def test_padding_lanes_under_the_open_threshold(O, base):
    order = _probe_order(O, base['cen'], base['xq'][1])
    sizes = [1, 33, 63]
    assign = _assign_by_rank(order, sizes)
    x = base['xb'][500:500 + sum(sizes)]
    xq = np.concatenate([base['xq'][:N_REG], np.zeros((1, D), np.float32), -base['xb'][510][None]])
    res, _, _ = _both_layouts_and_oracle(O, base, x, assign, xq, (1024,))
    Io = res[1024][1]
    assert (Io[:, 97:] == -1).all()                        # exactly the stored vectors, then the padding
    assert (np.sort(Io[:, :97], axis=1) == np.arange(97)[None]).all()


def test_the_key_of_slot_zero_with_score_zero_is_not_an_empty_slot(O, base):
    n = 300
    assign = (np.arange(n) % 5).astype(np.int32)           # vector 0 is the first of list 0: tile 0, lane 0
    x = base['xb'][900:900 + n]
    xq = np.concatenate([np.zeros((1, D), np.float32), base['xq'][:N_REG]])
    res, _, idx = _both_layouts_and_oracle(O, base, x, assign, xq, (1, 8, 1024))
    _stored_in_order(idx, 0, np.arange(0, n, 5))
    for k in (1, 8, 1024):
        Do, Io = res[k]
        m = min(k, n)
        assert np.array_equal(Io[0][:m], np.arange(m)) and (_bits(Do[0][:m]) == 0).all()   # +0.0, ties by id


def test_negative_scores_when_exact_flushes_take_over(O, base):
    xdup = base['xb'][9]
    order = _probe_order(O, base['cen'], xdup)
    front = [64, 7, 33, 64, 2]
    sizes = front + [DUP_N]                                # the copies probed last
    assign = _assign_by_rank(order, sizes)
    n = len(assign)
    x = base['xb'][100:100 + n].copy()
    dup_rows = np.arange(sum(front), n)
    x[dup_rows] = xdup
    xq = np.concatenate([xdup[None], -xdup[None], np.zeros((1, D), np.float32), base['xq'][:N_REG]])
    perm = np.random.default_rng(SEED + 400).permutation(n)
    res, _, _ = _both_layouts_and_oracle(O, base, x[perm], assign[perm], xq, (1024, 1500))
    dup_id = np.nonzero(np.isin(perm, dup_rows))[0]
    for k in (1024, 1500):
        Do, Io = res[k]
        hit = np.isin(Io[0], dup_id)                       # more equal scores than either buffer's free room
        assert hit[-1] and hit.sum() > 900 and len(np.unique(_bits(Do[0][hit]))) == 1
        neg = np.isin(Io[1], dup_id)                       # the copies are the LOWEST of the negated query
        assert (Do[1] < 0).sum() > 900 and neg[-1] and neg.sum() > 500 and len(np.unique(_bits(Do[1][neg]))) == 1


def test_two_probes_per_thread(O, base, lengths):
    nlist = 600
    cen = np.ascontiguousarray(base['xb'][np.random.default_rng(SEED + 5).choice(len(base['xb']), nlist, replace=False)])
    x, assign = lengths(300, nlist)
    xq = np.concatenate([base['xq'][:N_REG + 2], np.zeros((1, D), np.float32)])
    _both_layouts_and_oracle(O, base, x, assign, xq, (64, 1024, 1500), nlist=nlist, cen=cen)


def test_the_selected_scan(O, base, lengths):
    x, assign = lengths(300)
    xq = base['xq'][:N_REG + 3]
    ivf = O.HostIVF(base['cen'], assign, O.pq_encode(x, base['cen'], assign, base['cb']), base['cb'])
    idx = _index(base['cen'], base['cb'], x, assign, NLIST)
    keep = np.arange(len(x)) % 2 == 0                      # every other vector: half of most tiles' lanes
    idx.set_selector(keep)
    try:
        for k in (8, 1024):
            got = idx.search_selected(xq, k)
            SR.assert_rows_equal(got, SR.search_selected(O, ivf, xq, k, NLIST, keep), k)
            hit = got[1][got[1] >= 0]
            assert keep[hit].all() and len(hit)
    finally:
        idx.set_selector(None)


def test_the_window_scan(O, base):
    w_nlist = 64
    sizes = np.array([168] * 54 + [100, 30, 200] + [0] * 7, np.int64)
    windows = ((0, 63), (1, 64), (63, 128), (31, 32))      # ranks [a, b]: runs that start and end inside a tile
    assert [_window_entries(sizes, a, b) for a, b in windows] == [57, 113, 167, 56]
    n = int(sizes.sum())
    assign = np.random.default_rng(SEED + 2).permutation(np.repeat(np.arange(w_nlist, dtype=np.int32), sizes))
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
    for k in (8, 1024):
        got = idx.search_window(xq, k, wins, 2, 0.0, 'interval')
        IR.assert_rows_equal(got, IR.index_rows(O, ivf, xq, k, w_nlist, key, wins))
        assert (got[1][:, 0] >= 0).all()


def test_set_mode_rows_with_the_scan_side_precursor_filter(O):
    from ann_solo_amd import _lib, synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, aux = synthetic.make_library(2500, seed=713, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, 48, seed=714, charge=2)
    cfg = Config.open_search(num_list=8, num_probe=8, num_candidates=64, index='ivfpq', kmeans_niter=3,
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
