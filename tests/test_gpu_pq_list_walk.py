"""The sub-quantiser-major IVF-PQ scan hands out whole lists to its waves from a per-probe table.

Its instantiations keep one 16-byte entry per probe (first tile, length, coarse term), 128 probes per chunk; a wave
takes the chunk's next list by a ticket counter, draws the ticket for the list after it when it starts fetching the
current one, skips entries of length 0, makes every tile's entry by scalar arithmetic from the list's, and is finished
when no ticket is left and its pipeline is empty. What that can break: fewer, as many and more non-empty lists than
waves; the chunk of 128 probes, a chunk of one probe, two probes per thread; the last tile of a list at every
fill; a list advance with every step; look-ahead tickets that land on empty lists; a refused reservation while the
lists advance; and the dispatcher's edge (nprobe < 32 takes the tile table).

The indexes: d = 800, m = 32, 8 bits, filled through asl_index_add_preassigned with nprobe = nlist, so that every
list is probed and the list sizes alone say what a query walks (in the order of ITS coarse scores). Variant 0 (the
list walk, from nprobe 32 on), variant 2 (the tile table, tile-major codes) and the oracle: ids and score bits equal,
no tolerance, at k = 1024 (2048-key instantiation) and k = 1500 (4096 keys).

The set-mode case goes through SpectralLibrary, which trains its own quantiser (a preassigned index cannot be given
to it): 64 lists of about one tile each, all probed, 47 queries, the scan-side precursor filter on; variant 0
against variant 2."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, M, NITER, SEED = 800, 32, 2, 9127
DSUB = D // M
N_MAX, NCEN = 12000, 600
KS = (1024, 1500)
NQ = 40
Q_ZERO, Q_ONE, Q_LOW16, Q_DUP = range(4)
LENGTHS = (0, 1, 63, 64, 65, 128, 129)
DUP_N = 3000
NONEMPTY = (0, 1, 7, 8, 9)                   # fewer than, as many as and more than the eight waves
NPROBES = (31, 32, 127, 128, 129, 257, 600)  # the dispatcher's edge; the chunk of 128 probes; two probes per thread
DUP_AT = ('first', 'last', 'only')
CASES = [('nonempty', c) for c in NONEMPTY] + [('nprobe', n) for n in NPROBES] + [('onetile', 128)] + \
        [('dup', w) for w in DUP_AT]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _sparse_row(rng, dims):
    x = np.zeros(D, np.float32)
    x[dims] = rng.random(len(dims)).astype(np.float32) + 0.1
    return x / np.float32(np.sqrt((x.astype(np.float64) ** 2).sum()))


def _mixed(nlist, rng, budget):
    """Every length of LENGTHS (as often as the lists allow, six times at the most), a list of several tiles
    every 32 lists, the rest a few vectors or none; shuffled over the lists."""
    sizes = []
    for i in range(nlist):
        if i < 7 * min(6, max(1, nlist // 8)):
            sizes.append(LENGTHS[i % 7])
        elif i % 32 == 31:
            sizes.append(int(rng.integers(150, 400)))
        else:
            sizes.append(int(rng.choice([0, 1, 2, 5, 1, 0, 7, 1])))
    sizes = np.array(sizes, np.int64)
    assert sizes.sum() <= budget and set(LENGTHS) <= set(sizes.tolist())
    return sizes[rng.permutation(nlist)]


def _plan(kind, arg, rng, dup_rank):
    """(nlist, sizes, dup list or -1)."""
    if kind == 'nonempty':
        sizes = np.zeros(128, np.int64)
        sizes[rng.choice(128, arg, replace=False)] = [129, 1, 63, 64, 65, 128, 700, 64, 130][:arg]
        return 128, sizes, -1
    if kind == 'nprobe':
        return arg, _mixed(arg, rng, N_MAX), -1
    if kind == 'onetile':
        sizes = rng.integers(1, 65, arg)
        sizes[:3] = (1, 63, 64)
        return arg, sizes[rng.permutation(arg)], -1
    order, tail = dup_rank(128)                 # the lists in the order Q_DUP probes them; those tied for the last place
    dup = int(tail[0] if arg == 'last' else order[0])
    sizes = np.zeros(128, np.int64) if arg == 'only' else _mixed(128, rng, N_MAX - DUP_N)
    if arg == 'last':                           # (whatever the order among the tied, the other probes there are empty)
        sizes[tail] = 0
    sizes[dup] = DUP_N
    return 128, sizes, dup


@pytest.fixture(scope='module')
def world(O):
    """The vectors, the quantisers and the queries; per case the list sizes, the assignment, the oracle's inverted
    lists (checked to hold the planned sizes), the index and the oracle's answers, each made once."""
    from ann_solo_amd import synthetic
    rng = np.random.default_rng(SEED)
    lib, aux = synthetic.make_library(N_MAX, seed=613, device='cpu')
    q, _ = synthetic.make_queries(lib, aux, NQ, seed=614)
    o, mz, inten, *_ = lib.numpy()
    xb = O.encode_batch(mz, inten, o, 10.96, 0.04, D)
    o, mz, inten, *_ = q.numpy()
    xq = O.encode_batch(mz, inten, o, 10.96, 0.04, D)
    cen = np.ascontiguousarray(xb[rng.choice(N_MAX, NCEN, replace=False)])
    cb = O.pq_train(xb[:4000], cen, M, 256, NITER, SEED + 7)
    xq[Q_ZERO] = 0.0
    xq[Q_ONE] = _sparse_row(rng, 21 * DSUB + np.array([0, 11, 24]))
    xq[Q_LOW16] = _sparse_row(rng, np.array([m * DSUB + (m * 5) % DSUB for m in range(16)]))
    dup_vec = xb[N_MAX - 1].copy()
    xq[Q_DUP] = dup_vec
    live = [set((np.nonzero(r)[0] // DSUB).tolist()) for r in xq]
    assert live[Q_ZERO] == set() and live[Q_ONE] == {21} and live[Q_LOW16] == set(range(16))

    def dup_rank(nlist):
        ip = cen[:nlist].astype(np.float64) @ dup_vec.astype(np.float64)
        order = np.argsort(-ip, kind='stable')
        assert ip[order[0]] > ip[order[1]]                                       # no tie for the first place
        return order, np.nonzero(ip == ip.min())[0]
    made = {}

    def case(kind, arg):
        key = (kind, arg)
        if key not in made:
            crng = np.random.default_rng([SEED, CASES.index(key)])
            nlist, sizes, dup = _plan(kind, arg, crng, dup_rank)
            n = int(sizes.sum())
            assert n <= N_MAX
            assign = crng.permutation(np.repeat(np.arange(nlist, dtype=np.int32), sizes))
            x = xb[:n].copy()
            if dup >= 0:
                x[assign == dup] = dup_vec
            c = np.ascontiguousarray(cen[:nlist])
            ivf = O.HostIVF(c, assign, O.pq_encode(x, c, assign, cb) if n else np.zeros((0, M), np.uint8), cb)
            assert np.array_equal(np.diff(ivf.list_offsets), sizes)             # the plan, by the oracle alone
            made[key] = dict(nlist=nlist, sizes=sizes, dup=dup, assign=assign, ivf=ivf, idx=_index(c, cb, x, assign, nlist),
                             answers={k: ivf.search(xq, k, nlist) for k in KS})
        return made[key]
    return dict(xq=xq, case=case, dup_rank=dup_rank)


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


@pytest.mark.parametrize('kind,arg', CASES)
def test_list_walk_tile_table_and_oracle_agree(world, kind, arg):
    c, xq = world['case'](kind, arg), world['xq']
    idx, sizes = c['idx'], c['sizes']
    assert idx.nprobe == c['nlist']
    if kind == 'nonempty':
        assert (sizes > 0).sum() == arg
        # 128 - arg empty probes in arg + 1 gaps of any probe order: a run of nine or more, whatever the query
        assert arg == 0 or (128 - arg) // (arg + 1) >= 9
    if kind == 'onetile':
        assert ((sizes >= 1) & (sizes <= 64)).all() and {1, 63, 64} <= set(sizes.tolist())
    if kind == 'dup':
        order, tail = world['dup_rank'](128)
        assert sizes[c['dup']] == DUP_N
        if arg == 'last':                 # the only non-empty list among those tied for the last place
            assert c['dup'] in tail and (sizes[tail] > 0).sum() == 1
        else:
            assert c['dup'] == order[0]
        assert ((sizes > 0).sum() == 1) == (arg == 'only')
    for k in KS:
        Do, Io = c['answers'][k]
        idx.set_scan_variant(2)
        Dt, It = idx.search(xq, k)
        idx.set_scan_variant(0)
        Dm, Im = idx.search(xq, k)
        assert idx.codes_mmajor or sizes.sum() == 0
        assert np.array_equal(Im, It) and np.array_equal(_bits(Dm), _bits(Dt)), k
        assert np.array_equal(Im, Io) and np.array_equal(_bits(Dm), _bits(Do)), k
    if sizes.sum() == 0:
        assert (Io == -1).all()
    if kind == 'dup':                     # k cuts through the block of equal scores, larger than the key buffer
        Do, Io = c['answers'][1024]
        dup = np.isin(Io[Q_DUP], np.nonzero(c['assign'] == c['dup'])[0])
        assert dup[-1] and dup.sum() > 900 and len(np.unique(Do[Q_DUP][dup])) == 1


def test_set_mode_batch_with_the_scan_side_filter_at_an_odd_batch_size():
    from ann_solo_amd import _lib, synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, aux = synthetic.make_library(3000, seed=713, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, 47, seed=714, charge=2)
    cfg = Config.open_search(num_list=64, num_probe=64, num_candidates=256, index='ivfpq', kmeans_niter=3,
                             precursor_tolerance_mass_open=500, precursor_tolerance_mode_open='Da')
    prev = _lib.lib().asl_set_scan_postfilter(1)
    sl = SpectralLibrary(lib, config=cfg, device='cuda:0')
    try:
        idx = sl._get_ann_index(2)
        assert idx.info().nlist == 64
        idx.set_scan_variant(2)
        ref = sl._search_batch(q, 2, 'open')
        idx.set_scan_variant(0)
        r = sl._search_batch(q, 2, 'open')
        assert (ref.best_row >= 0).mean() > 0.5
        assert np.array_equal(r.best_row, ref.best_row)
        assert np.array_equal(r.best_score, ref.best_score)
        assert np.array_equal(r.n_candidates, ref.n_candidates)
        assert np.array_equal(r.pm_count, ref.pm_count)
    finally:
        sl.shutdown()
        _lib.lib().asl_set_scan_postfilter(prev)
