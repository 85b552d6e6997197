"""The tiled IVF-PQ scan at the end of a wave's share of the tile table and in the lanes of dead sub-quantisers.

The tile loop of the sub-quantiser-major scan prefetches the codes of the next tile unconditionally: past the
end of a wave's share it fetches the chunk's last entry again (never scored), and a lane whose sub-quantiser has
no non-zero query component issues its loads out of the buffer's range, which returns zeros. What that can
break is the end of a share (fewer entries than waves, every position of the last entry in the rotation of the
two register sets, a chunk of exactly 256 entries, a further chunk of one entry, a third chunk) and the dead
lanes. The tile-major, window and selected scans keep the conditional fetch; the same ends of a share are checked
in them. The ADC itself is covered elsewhere.

The indexes: d = 800, m = 32, 8 bits, 512 lists filled through asl_index_add_preassigned, nprobe = nlist, so
that a query's tile table is the whole index and its length is set by the list sizes: 0, 1, 7, 8, 9, 15, 16, 17,
255, 256, 257 and 513 tiles, most lists a tile or two with last tiles of 1, 63, 64 and other counts, two of
the indexes with a list of 3 000 copies of ONE vector (refused reservations and syncs anywhere in a share).
The default scan (sub-quantiser-major) and variant 2 (tile-major) against each other and against the oracle:
ids and score bits equal, no tolerance; k = 1024 (2048-key instantiation) and k = 1500 (4096 keys). The window
scan (12-byte entries, 168 per chunk) at 167, 168 and 169 entries with the first and the last tile of every
run partial, the selected scan on both sides of a chunk boundary, and 600 lists with nprobe = 600 (two probes per
thread, the WIDE instantiations of both layouts and both key buffers) at 9 and 257 tiles."""
import ctypes as C

import numpy as np
import pytest

import interval_ref as IR
import selector_ref as SR

pytestmark = pytest.mark.gpu

D, M, NLIST, NITER, SEED = 800, 32, 512, 2, 4421
DSUB = D // M
TOTALS = (0, 1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 513)
DUP_IN, DUP_N = (255, 257), 3000           # the indexes that hold the list of copies (47 tiles)
KS = (1024, 1500)
NQ = 40
Q_ZERO, Q_ONE_HI, Q_ONE_LO, Q_ALL, Q_LOW16, Q_HIGH16, Q_DUP = range(7)
WIDE_NLIST, WIDE_TOTALS = 600, (9, 257)     # nprobe > 512: two probes per thread
# the window-scan index: 64 lists, rank r of a vector in its list is its key 500 + r
W_NLIST = 64
W_SIZES = [168] * 54 + [100, 30, 200] + [0] * 7
W_WINDOWS = ((5, 150), (40, 150), (5, 195), (40, 195))      # ranks [a, b] -> 168, 167, 169, 168 entries


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _sizes(total, rng, nlist=None):
    """List sizes (512 of them, or `nlist`, most empty) whose tiles add up to `total`."""
    nlist = nlist or NLIST
    sizes, left = [], total
    if total in DUP_IN:
        sizes.append(DUP_N)
        left -= (DUP_N + 63) // 64
    last = [1, 63, 64]                      # the first lists end in tiles of 1, 63 and 64 vectors
    while left > 0:
        nt = min(left, int(rng.choice([1] * 8 + [2, 3])))
        fill = last.pop(0) if last else int(rng.choice([1, 3, 7, 16, 63, 64], p=[.4, .25, .2, .09, .03, .03]))
        sizes.append(64 * (nt - 1) + fill)
        left -= nt
    assert len(sizes) <= nlist - 1          # at least one empty list
    sizes += [0] * (nlist - len(sizes))
    return np.array(sizes, np.int64)[rng.permutation(nlist)]


def _sparse_row(rng, dims):
    x = np.zeros(D, np.float32)
    x[dims] = rng.random(len(dims)).astype(np.float32) + 0.1
    return x / np.float32(np.sqrt((x.astype(np.float64) ** 2).sum()))


def _tiles(sizes):
    return int(((np.asarray(sizes) + 63) // 64).sum())


def _window_entries(sizes, a, b):
    """Entries of the window scan's tile table for the ranks [a, b] of every list."""
    s = np.asarray(sizes)
    hi = np.minimum(b, s - 1)
    return int(np.where(s > a, (hi >> 6) - (a >> 6) + 1, 0).sum())


@pytest.fixture(scope='module')
def world(O):
    """The vectors, the quantisers and the queries, and per table length the list sizes, the assignment, the
    oracle's inverted lists (checked to hold the stated number of tiles) and its answers, computed once."""
    from ann_solo_amd import synthetic
    rng = np.random.default_rng(SEED)
    plans = {t: _sizes(t, rng) for t in TOTALS}
    n_max = max(max(int(s.sum()) for s in plans.values()), sum(W_SIZES))
    assert n_max <= 12000
    lib, aux = synthetic.make_library(n_max, seed=271, device='cpu')
    q, _ = synthetic.make_queries(lib, aux, NQ, seed=272)
    o, mz, inten, *_ = lib.numpy()
    xb = O.encode_batch(mz, inten, o, 10.96, 0.04, D)
    o, mz, inten, *_ = q.numpy()
    xq = O.encode_batch(mz, inten, o, 10.96, 0.04, D)
    cen = np.ascontiguousarray(xb[rng.choice(n_max, NLIST, replace=False)])
    cb = O.pq_train(xb[:4000], cen, M, 256, NITER, SEED + 7)
    xq[Q_ZERO] = 0.0
    xq[Q_ONE_HI] = _sparse_row(rng, 21 * DSUB + np.array([0, 11, 24]))
    xq[Q_ONE_LO] = _sparse_row(rng, 6 * DSUB + np.array([3, 9]))
    xq[Q_ALL] = _sparse_row(rng, np.array([m * DSUB + (m * 7) % DSUB for m in range(M)]))
    xq[Q_LOW16] = _sparse_row(rng, np.array([m * DSUB + (m * 5) % DSUB for m in range(16)]))
    xq[Q_HIGH16] = _sparse_row(rng, np.array([m * DSUB + (m * 3) % DSUB for m in range(16, 32)]))
    live = [set((np.nonzero(r)[0] // DSUB).tolist()) for r in xq]
    assert live[Q_ZERO] == set() and live[Q_ONE_HI] == {21} and live[Q_ONE_LO] == {6}
    assert live[Q_ALL] == set(range(32)) and live[Q_LOW16] == set(range(16)) and live[Q_HIGH16] == set(range(16, 32))
    rest = np.arange(NQ) > Q_DUP
    assert rest.sum() >= 30 and ((xq[rest] != 0).sum(1) <= 64).all()      # hashed rows: the entry-list path
    assert any(0 < len(live[i]) < M for i in np.nonzero(rest)[0])         # ... with dead sub-quantisers
    cases = {}

    def case(total):
        if total not in cases:
            sizes = plans[total]
            n = int(sizes.sum())
            assign = np.random.default_rng(SEED + total).permutation(np.repeat(np.arange(NLIST, dtype=np.int32), sizes))
            x = xb[:n].copy()
            xqc = xq.copy()
            if total in DUP_IN:
                rows = np.nonzero(assign == int(np.argmax(sizes)))[0]
                assert len(rows) == DUP_N
                x[rows] = x[rows[0]]
                xqc[Q_DUP] = x[rows[0]]
            ivf = O.HostIVF(cen, assign, O.pq_encode(x, cen, assign, cb) if n else np.zeros((0, M), np.uint8), cb)
            size = np.diff(ivf.list_offsets)
            assert _tiles(size) == total and (size == 0).any()            # the table's length, by the oracle alone
            if total >= 7:                  # vectors in a list's last tile
                assert {1, 63, 64} <= set(((size[size > 0] - 1) % 64 + 1).tolist())
            cases[total] = dict(x=x, xq=xqc, assign=assign, ivf=ivf, answers={})
        return cases[total]

    def oracle(total, k):
        c = case(total)
        if k not in c['answers']:
            c['answers'][k] = c['ivf'].search(c['xq'], k, NLIST)
        return c['answers'][k]
    return dict(xb=xb, xq=xq, cen=cen, cb=cb, case=case, oracle=oracle)


def _index(cen, cb, x, assign, nlist):
    from ann_solo_amd import _lib
    from ann_solo_amd import faiss_compat as faiss
    idx = faiss.IndexIVFPQ(faiss.IndexFlatIP(D), D, nlist, M, 8)
    idx.set_trained(cen, cb)
    if len(x):
        x = np.ascontiguousarray(x, np.float32)
        assign = np.ascontiguousarray(assign, np.int32)
        _lib.check(_lib.lib().asl_index_add_preassigned(idx._h, C.c_int64(len(x)), x.ctypes.data_as(C.c_void_p),
                                                        assign.ctypes.data_as(C.c_void_p)))
    idx.nprobe = nlist
    return idx


@pytest.fixture(scope='module')
def indexes(world):
    made = {}

    def get(total):
        if total not in made:
            c = world['case'](total)
            made[total] = _index(world['cen'], world['cb'], c['x'], c['assign'], NLIST)
        return made[total]
    return get


@pytest.mark.parametrize('total', TOTALS)
def test_both_code_layouts_and_the_oracle_agree_at_every_table_length(world, indexes, total):
    c, idx = world['case'](total), indexes(total)
    for k in KS:
        Do, Io = world['oracle'](total, k)
        idx.set_scan_variant(2)
        Dt, It = idx.search(c['xq'], k)
        idx.set_scan_variant(0)
        Dm, Im = idx.search(c['xq'], k)
        assert idx.codes_mmajor or total == 0
        assert np.array_equal(Im, It) and np.array_equal(_bits(Dm), _bits(Dt)), k
        assert np.array_equal(Im, Io) and np.array_equal(_bits(Dm), _bits(Do)), k
    if total == 0:
        assert (Io == -1).all()
    if total in DUP_IN:                   # k cuts through the block of equal scores, larger than the key buffer
        Do, Io = world['oracle'](total, 1024)
        dup = np.isin(Io[Q_DUP], np.nonzero(c['assign'] == int(np.argmax(np.bincount(c['assign']))))[0])
        assert dup[-1] and dup.sum() > 900 and len(np.unique(Do[Q_DUP][dup])) == 1


@pytest.fixture(scope='module')
def window_world(O, world):
    sizes = np.array(W_SIZES, np.int64)
    n = int(sizes.sum())
    rng = np.random.default_rng(SEED + 1)
    assign = rng.permutation(np.repeat(np.arange(W_NLIST, dtype=np.int32), sizes))
    cen = np.ascontiguousarray(world['cen'][:W_NLIST])
    x = world['xb'][:n]
    ivf = O.HostIVF(cen, assign, O.pq_encode(x, cen, assign, world['cb']), world['cb'])
    assert np.array_equal(np.sort(np.diff(ivf.list_offsets)), np.sort(sizes))
    # a vector's key: 500 + its rank in its list (the oracle's lists are in id order, and so is then the
    # window-ordered layout); ranks [a, b] are the interval [500 + a - 0.25, 500 + b + 0.25]
    key = np.empty(n, np.float32)
    for l in range(W_NLIST):
        ids = ivf.ids[ivf.list_offsets[l]:ivf.list_offsets[l + 1]]
        key[ids] = 500.0 + np.arange(len(ids), dtype=np.float32)
    entries = [_window_entries(sizes, a, b) for a, b in W_WINDOWS]
    assert entries == [168, 167, 169, 168]
    assert all(a & 63 and (b + 1) & 63 for a, b in W_WINDOWS)           # first and last tile of a run partial
    wins = np.array([[500.0 + W_WINDOWS[i % 4][0] - 0.25, 500.0 + W_WINDOWS[i % 4][1] + 0.25] for i in range(NQ)])
    return dict(idx=_index(cen, world['cb'], x, assign, W_NLIST), ivf=ivf, key=key, wins=wins)


def test_window_scan_around_its_chunk_of_168_entries(O, world, window_world):
    w = window_world
    w['idx'].set_window_key(w['key'])
    k = 1024
    got = w['idx'].search_window(world['xq'], k, w['wins'], 2, 0.0, 'interval')
    IR.assert_rows_equal(got, IR.index_rows(O, w['ivf'], world['xq'], k, W_NLIST, w['key'], w['wins']))
    assert (got[1][:, 0] >= 0).all()


@pytest.mark.parametrize('total', [256, 257])
def test_selected_scan_on_both_sides_of_a_chunk_boundary(O, world, indexes, total):
    c, idx = world['case'](total), indexes(total)
    keep = np.arange(len(c['x'])) % 3 != 1
    idx.set_selector(keep)
    try:
        for k in (64, 1024):
            got = idx.search_selected(c['xq'], k)
            SR.assert_rows_equal(got, SR.search_selected(O, c['ivf'], c['xq'], k, NLIST, keep), k)
            hit = got[1][got[1] >= 0]
            assert keep[hit].all() and len(hit)
    finally:
        idx.set_selector(None)


@pytest.fixture(scope='module')
def wide_world(O, world):
    """600 lists, every one probed: centroids of their own, the codebooks of the other indexes."""
    rng = np.random.default_rng(SEED + 2)
    cen = np.ascontiguousarray(world['xb'][rng.choice(len(world['xb']), WIDE_NLIST, replace=False)])
    out = {}
    for total in WIDE_TOTALS:
        sizes = _sizes(total, rng, WIDE_NLIST)
        n = int(sizes.sum())
        assign = rng.permutation(np.repeat(np.arange(WIDE_NLIST, dtype=np.int32), sizes))
        x = world['xb'][:n]
        ivf = O.HostIVF(cen, assign, O.pq_encode(x, cen, assign, world['cb']), world['cb'])
        assert _tiles(np.diff(ivf.list_offsets)) == total
        out[total] = dict(ivf=ivf, idx=_index(cen, world['cb'], x, assign, WIDE_NLIST))
    return out


@pytest.mark.parametrize('total', WIDE_TOTALS)
def test_two_probes_per_thread_at_the_end_of_a_share(world, wide_world, total):
    w, xq = wide_world[total], world['xq']
    assert w['idx'].nprobe == WIDE_NLIST > 512
    for k in KS:
        Do, Io = w['ivf'].search(xq, k, WIDE_NLIST)
        w['idx'].set_scan_variant(2)
        Dt, It = w['idx'].search(xq, k)
        w['idx'].set_scan_variant(0)
        Dm, Im = w['idx'].search(xq, k)
        assert w['idx'].codes_mmajor
        assert np.array_equal(Im, It) and np.array_equal(_bits(Dm), _bits(Dt)), k
        assert np.array_equal(Im, Io) and np.array_equal(_bits(Dm), _bits(Do)), k
