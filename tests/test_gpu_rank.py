"""asl_index_rank (faiss_compat rank_of, SpectralLibrary.candidate_rank): the rank of a given library
vector in the index's neighbour order, against the oracle's full-scope rows -- HostIVF.search at k = n
returns the whole scope in (score desc, id asc) order, so the expected rank is the target's position in
that row, -1 when absent. Exact integers and score bits throughout, no tolerance.

Shapes: the 5 000-spectrum tie library of test_gpu_window_scan (400 copies of row 0 spread over +-300 Da)
under nlist = 4 (lists longer than one 832-vector block and than several 64-vector tiles) and nlist = 16;
48 queries, 8 of them copies of row 0, one all-zero, one with more than 64 non-zeros."""
import numpy as np
import pytest

from rank_ref import expected_ranks
from test_gpu_window_scan import _queries, _tie_library, _window_mask

pytestmark = pytest.mark.gpu

N, NQ = 5000, 48
Q_ZERO, Q_DENSE = 47, 46
WINDOWS = [('key0', 250.0, 'Da'), ('key0', 2e5, 'ppm'), ('key0', 0.5, 'Da'), ('key0', -1.0, 'Da'),
           ('key0', 1e9, 'Da'), ('key_nan', 250.0, 'Da')]


def _host(O, idx):
    """The oracle's IVF over the device's own centroids, lists and payload (codes and codebooks for IVF-PQ)."""
    off, ids, payload = idx.lists()
    info = idx.info()
    ivf = O.HostIVF.__new__(O.HostIVF)
    ivf.centroids, ivf.nlist, ivf.d = idx.centroids(), info.nlist, info.d
    ivf.list_offsets, ivf.ids, ivf.payload = off, ids, payload
    ivf.kind = 1 if info.kind == 2 else 0
    ivf.codebooks = idx.codebooks() if info.kind == 2 else None
    return ivf


def _filtered(O, ivf, keep_by_id):
    """The oracle's IVF with only the vectors whose id is kept (test_gpu_window_scan._filtered, either kind)."""
    keep = keep_by_id[ivf.ids]
    lst = np.repeat(np.arange(ivf.nlist), np.diff(ivf.list_offsets))
    out = O.HostIVF.__new__(O.HostIVF)
    out.centroids, out.nlist, out.d, out.codebooks, out.kind = ivf.centroids, ivf.nlist, ivf.d, ivf.codebooks, ivf.kind
    out.list_offsets = np.concatenate([[0], np.cumsum(np.bincount(lst[keep], minlength=ivf.nlist))]).astype(np.int32)
    out.ids = np.ascontiguousarray(ivf.ids[keep])
    out.payload = np.ascontiguousarray(ivf.payload[keep])
    return out


def _special_ids(off, ids):
    """Per list: its first and last position, the last slot of its first block and the first of its second
    (832 vectors a block), lanes 63 and 0 of its first two tiles, the first lane of its last, partial tile."""
    out = []
    for l in range(len(off) - 1):
        a, n = int(off[l]), int(off[l + 1] - off[l])
        for r in (0, n - 1, 831, 832, 63, 64, (n - 1) // 64 * 64, 1):
            if 0 <= r < n:
                out.append(int(ids[a + r]))
    return list(dict.fromkeys(out))


class World:
    """One library, its queries and targets; indexes and the oracle's rows are made once and shared."""

    def __init__(self, O):
        from ann_solo_amd import synthetic
        self.O = O
        self.lib0, self.aux, self.lib = _tie_library(N)
        self.q = _queries(self.lib0, self.aux, NQ, seed=72, with_copies=8)
        _, truth = synthetic.make_queries(self.lib0, self.aux, NQ, seed=72, charge=2)
        self.source = truth['source_row'].cpu().numpy().astype(np.int64)
        self.source[:8] = 0
        self.q_pmz = self.q.numpy()[4].astype(np.float64)
        self.sl, self.host, self.rows, self.xq = {}, {}, {}, None

    def index(self, kind, nlist):
        from ann_solo_amd.spectral_library import Config, SpectralLibrary
        if (kind, nlist) not in self.sl:
            cfg = Config.open_search(num_list=nlist, num_probe=min(8, nlist), num_candidates=256, index=kind,
                                     kmeans_niter=4, precursor_tolerance_mass_open=250.0,
                                     precursor_tolerance_mode_open='Da')
            sl = SpectralLibrary(self.lib, config=cfg)
            self.sl[kind, nlist] = sl
            self.host[kind, nlist] = _host(self.O, sl._get_ann_index(2))
            if self.xq is None:
                xq = sl._encode(self.q.to(sl.device)).cpu().numpy()
                xq[Q_ZERO] = 0.0
                rng = np.random.default_rng(9)
                xq[Q_DENSE] = 0.0
                xq[Q_DENSE, rng.choice(xq.shape[1], 90, replace=False)] = rng.random(90).astype(np.float32) + 0.05
                xq[Q_DENSE] /= np.linalg.norm(xq[Q_DENSE])
                self.xq = np.ascontiguousarray(xq, np.float32)
                self.key0 = np.ascontiguousarray(sl.partitions[2].precursor_mz, np.float32)
                self.key_nan = self.key0.copy()
                self.key_nan[::7] = np.nan
        sl = self.sl[kind, nlist]
        return sl, sl._get_ann_index(2), self.host[kind, nlist]

    def full_rows(self, kind, nlist, nprobe, window=None):
        """(D, I) [NQ, N]: the oracle's whole scope per query, in neighbour order, -1 padded."""
        tag = (kind, nlist, nprobe, window)
        if tag not in self.rows:
            ivf = self.host[kind, nlist]
            if window is None:
                self.rows[tag] = ivf.search(self.xq, N, nprobe)
            else:
                key, tol, mode = window
                D, I = np.empty((NQ, N), np.float32), np.empty((NQ, N), np.int64)
                for i in range(NQ):
                    keep = _window_mask(self.q_pmz[i], getattr(self, key), 2, tol, mode)
                    D[i], I[i] = (a[0] for a in _filtered(self.O, ivf, keep).search(self.xq[i:i + 1], N, nprobe))
                self.rows[tag] = D, I
        return self.rows[tag]

    def targets(self, kind, nlist):
        """Target vectors [NQ] each: source rows, the tie block, the special positions, ids out of range."""
        ivf = self.host[kind, nlist]
        sp = _special_ids(ivf.list_offsets, ivf.ids)
        out = [self.source, (np.arange(NQ) * 37 % 400).astype(np.int64)]
        for j in range((len(sp) + NQ - 1) // NQ):
            out.append(np.array([sp[(j * NQ + i) % len(sp)] for i in range(NQ)], np.int64))
        bad = np.array([-1, N, N + 7, -5, 1 << 40, -(1 << 35)], np.int64)
        out.append(bad[np.arange(NQ) % len(bad)])
        return out

    def close(self):
        for sl in self.sl.values():
            sl.shutdown()


@pytest.fixture(scope='module')
def world(O):
    w = World(O)
    yield w
    w.close()


def _check(world, idx, kind, nlist, T, nprobe, window=None):
    """rank, score and scope of one call against the oracle's rows; returns the ranks."""
    np_eff = nlist if nprobe == 0 else nprobe
    rD, rI = world.full_rows(kind, nlist, np_eff, window)
    win = None
    if window is not None:
        win = (getattr(world, window[0]), world.q_pmz, 2, window[1], window[2])
    rank, score, scope = idx.rank_of(world.xq, T, nprobe, win)
    want = expected_ranks(rI, T)
    print(kind, nlist, nprobe, window, 'in scope:', int((want >= 0).sum()), 'max rank:', int(want.max()))
    assert np.array_equal(rank, want), (kind, nlist, nprobe, window, np.nonzero(rank != want)[0][:8], rank[:8], want[:8])
    assert np.array_equal(scope, (rI >= 0).sum(1)), (kind, nlist, nprobe, window)
    hit = want >= 0
    got_bits = score.view(np.uint32)[hit]
    assert np.array_equal(got_bits, rD[np.nonzero(hit)[0], want[hit]].view(np.uint32)), (kind, nlist, nprobe, window)
    assert np.isnan(score[~hit]).all()
    return rank


@pytest.mark.parametrize('kind,nlist', [('ivfflat', 4), ('ivfflat', 16), ('ivfpq', 4), ('ivfpq', 16)])
def test_rank_is_the_position_in_the_oracles_row(world, kind, nlist):
    sl, idx, ivf = world.index(kind, nlist)
    if kind == 'ivfflat':
        assert idx.flat_layout == 1                 # float postings
        assert np.diff(ivf.list_offsets).max() > (832 if nlist == 4 else 64)
    unprobed = 0
    for T in world.targets(kind, nlist):
        r_all = _check(world, idx, kind, nlist, T, 0)
        r_nl = _check(world, idx, kind, nlist, T, nlist)
        assert np.array_equal(r_all, r_nl)          # nprobe = 0 is every list
        valid = (T >= 0) & (T < N)
        assert ((r_all >= 0) == valid).all()
        # the all-zero query: every score is 0, the rank is the number of smaller ids in scope
        if valid[Q_ZERO]:
            assert r_all[Q_ZERO] == T[Q_ZERO]
        r2 = _check(world, idx, kind, nlist, T, 2)
        unprobed += int(((r2 < 0) & valid).sum())
        assert (r2[r2 >= 0] <= r_all[r2 >= 0]).all()
    assert unprobed > 0                              # targets in lists that two probes do not reach
    # nprobe defaults to the handle's
    idx.nprobe = 2
    r_def = idx.rank_of(world.xq, world.source)[0]
    idx.nprobe = min(8, nlist)
    assert np.array_equal(r_def, idx.rank_of(world.xq, world.source, 2)[0])


@pytest.mark.parametrize('kind,nlist', [('ivfflat', 4), ('ivfflat', 16), ('ivfpq', 4), ('ivfpq', 16)])
def test_rank_inside_the_precursor_window(world, kind, nlist):
    sl, idx, ivf = world.index(kind, nlist)
    T_tie, T_src = world.targets(kind, nlist)[1], world.source
    plain = {id(T): idx.rank_of(world.xq, T, 0) for T in (T_tie, T_src)}
    inside = 0
    for w in WINDOWS:
        for T in (T_tie, T_src):
            rank = _check(world, idx, kind, nlist, T, 0, w)
            inside += int((rank >= 0).sum())
            if w[1] < 0:                             # the window passes nothing
                assert (rank == -1).all()
            if w[1] == 1e9:                          # the window passes everything: no window
                r0, s0, c0 = plain[id(T)]
                r1, s1, c1 = idx.rank_of(world.xq, T, 0, (world.key0, world.q_pmz, 2, 1e9, 'Da'))
                assert np.array_equal(r0, r1) and np.array_equal(c0, c1)
                assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32))
            if w[0] == 'key_nan':                    # a NaN key is never in scope
                assert (rank[np.isnan(world.key_nan[T])] == -1).all()
    assert inside > 0
    _check(world, idx, kind, nlist, T_tie, 2, WINDOWS[0])      # probes and window together
    _check(world, idx, kind, nlist, T_src, 2, WINDOWS[5])


@pytest.mark.parametrize('kind', ['ivfflat', 'ivfpq'])
def test_search_holds_the_target_from_rank_plus_one_on(world, kind):
    sl, idx, ivf = world.index(kind, 16)
    idx.nprobe = 8
    checked = 0
    for T in (world.source, world.targets(kind, 16)[1]):
        rank, score, _ = idx.rank_of(world.xq, T, 8)
        for i in np.nonzero((rank >= 0) & (rank < 1024))[0]:
            r = int(rank[i])
            D, I = idx.search(world.xq[i:i + 1], r + 1)
            assert I[0, r] == T[i] and D[0, r:].view(np.uint32)[0] == score[i:i + 1].view(np.uint32)[0], (kind, i, r)
            if r > 0:
                assert T[i] not in idx.search(world.xq[i:i + 1], r)[1][0], (kind, i, r)
            checked += 1
    assert checked > NQ


def test_device_tensors_and_candidate_rank(world):
    import torch
    for kind in ('ivfflat', 'ivfpq'):
        sl, idx, ivf = world.index(kind, 16)
        for nprobe in (None, 0):
            want = idx.rank_of(world.xq, world.source, 8 if nprobe is None else 0)
            got = idx.rank_of(torch.as_tensor(world.xq, device='cuda:0'), torch.as_tensor(world.source, device='cuda:0'),
                              8 if nprobe is None else 0)
            for a, b in zip(want, got):
                assert np.array_equal(a, b.cpu().numpy(), equal_nan=True)
        # the library-level call encodes the queries itself (the unmodified ones) and takes num_probe,
        # the open-level tolerance and the partition's precursor column from the library
        sel = np.arange(8, 40)
        xq = sl._encode(world.q.to(sl.device)).cpu().numpy()
        for window in (False, True):
            win = (world.key0, world.q_pmz, 2, 250.0, 'Da') if window else None
            want = idx.rank_of(xq, world.source, 8, win)
            got = sl.candidate_rank(world.q, 2, world.source, window=window)
            for a, b in zip(want, got):
                assert np.array_equal(a[sel], b[sel], equal_nan=True)
        r0 = sl.candidate_rank(world.q, 2, world.source, nprobe=0)[0]
        assert (r0[sel] >= 0).all()
        assert sl.candidate_rank(world.q, 7, world.source) is None


def test_a_rank_call_between_pipelined_batches(world):
    FIELDS = ('best_row', 'best_score', 'n_candidates', 'pm_count', 'pm_pairs')
    for kind in ('ivfflat', 'ivfpq'):
        sl, idx, ivf = world.index(kind, 16)
        ref = sl._search_batch(world.q, 2, 'open')
        want = idx.rank_of(world.xq, world.source, 0)
        sl.set_pipeline(True)
        try:
            qd = world.q.to('cuda:0')
            a = sl._search_batch(qd, 2, 'open', device_out=True)
            got = idx.rank_of(world.xq, world.source, 0)
            b = sl._search_batch(qd, 2, 'open', device_out=True)
            sl.synchronize()
        finally:
            sl.set_pipeline(False)
        for r in (a, b):
            for f in FIELDS:
                assert np.array_equal(getattr(r, f).cpu().numpy().astype(getattr(ref, f).dtype), getattr(ref, f)), (kind, f)
        for x, y in zip(want, got):
            assert np.array_equal(x, y, equal_nan=True)


def test_unsupported_cases_are_errors():
    from ann_solo_amd import _lib, faiss_compat as faiss
    L = _lib.lib()
    rng = np.random.default_rng(3)
    x = np.zeros((3000, 800), np.float32)
    for i in range(len(x)):
        x[i, rng.choice(800, 20, replace=False)] = rng.random(20) * 0.9 + 0.05
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    t = np.arange(8, dtype=np.int64)

    def made(index):
        index.set_niter(3)
        index.train(x)
        index.add(x)
        index.nprobe = 4
        return index

    ok = made(faiss.IndexIVFFlat(faiss.IndexFlatIP(800), 800, 8))
    rank, score, scope = ok.rank_of(x[:8], t, 0)
    assert (rank >= 0).all() and (scope == len(x)).all()
    # null arguments: ASL_ERR_INVALID
    r = np.zeros(8, np.int64)
    key = np.zeros(len(x), np.float32)
    args = lambda xq, tt, rr, kk=None, pp=None, nprobe=0, mode=0: L.asl_index_rank(
        ok._h, 8, _lib.ptr(xq), _lib.ptr(tt), nprobe, _lib.ptr(kk), _lib.ptr(pp), 2, 1.0, mode, _lib.ptr(rr), None, None)
    assert args(x[:8], t, r) == 0
    assert args(None, t, r) == -1 and args(x[:8], None, r) == -1 and args(x[:8], t, None) == -1
    assert args(x[:8], t, r, key, None) == -1                   # a key without precursor m/z
    assert args(x[:8], t, r, key, np.zeros(8), mode=5) == -1
    assert args(x[:8], t, r, nprobe=-1) == -1
    assert L.asl_index_rank(None, 8, _lib.ptr(x[:8]), _lib.ptr(t), 0, None, None, 2, 1.0, 0, _lib.ptr(r), None, None) == -1
    # fixed-point postings
    fx = made(faiss.IndexIVFFlat(faiss.IndexFlatIP(800), 800, 8, storage='fx22'))
    assert fx.flat_layout == 2
    with pytest.raises(_lib.AnnSoloMiError):
        fx.rank_of(x[:8], t, 0)
    # dense rows: no postings
    xd = rng.random((600, 800)).astype(np.float32)
    dense = faiss.IndexIVFFlat(faiss.IndexFlatIP(800), 800, 4)
    dense.set_niter(2)
    dense.train(xd)
    dense.add(xd)
    assert dense.flat_layout == 0
    with pytest.raises(_lib.AnnSoloMiError):
        dense.rank_of(xd[:8], t, 0)
    # a Flat index
    flat = faiss.IndexFlatIP(800)
    flat.add(x)
    with pytest.raises(_lib.AnnSoloMiError):
        flat.rank_of(x[:8], t, 0)
    # IVF-PQ: the generic variant, a generic shape, a sharded index
    pq = made(faiss.IndexIVFPQ(faiss.IndexFlatIP(800), 800, 8, 32, 8))
    assert (pq.rank_of(x[:8], t, 0)[0] >= 0).all()
    pq.set_scan_variant(1)
    with pytest.raises(_lib.AnnSoloMiError):
        pq.rank_of(x[:8], t, 0)
    pq.set_scan_variant(0)
    pq16 = made(faiss.IndexIVFPQ(faiss.IndexFlatIP(800), 800, 8, 16, 8))
    with pytest.raises(_lib.AnnSoloMiError):
        pq16.rank_of(x[:8], t, 0)
    pq.shard(0, 2)
    with pytest.raises(_lib.AnnSoloMiError):
        pq.rank_of(x[:8], t, 0)
    ok.shard(0, 2)
    with pytest.raises(_lib.AnnSoloMiError):
        ok.rank_of(x[:8], t, 0)
