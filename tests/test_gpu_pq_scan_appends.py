"""The tiled IVF-PQ scan with free-running appends (csrc/pq_scan_v3.hip): the waves of a workgroup
append on their own and meet only when the key buffer is full and at the end of a table chunk.
Every case below makes the protocol work -- with k >= 1024 a query fills the 2048-key buffer within
its first 32 tiles, so syncs happen in the middle of a chunk -- and compares ids AND score bits with
the oracle's IVF-PQ search over the same stored codes, never with the kernel's own output."""
import numpy as np
import pytest
import torch      # before the C library is loaded, as everywhere in the package: one HIP runtime per process

pytestmark = pytest.mark.gpu

DIM = 800
N = 26000            # 407 tiles of 64 vectors: more than one 256-entry table chunk per query
NLIST = 40
NQ = 40


def _rows(rng, n, lo=15, hi=45):
    """sparse, non-negative unit vectors (the shape of hashed spectra)"""
    x = np.zeros((n, DIM), np.float32)
    for i in range(n):
        c = rng.choice(DIM, size=int(rng.integers(lo, hi + 1)), replace=False)
        x[i, c] = (rng.random(len(c)) + 0.05).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _queries(rng, x, nq):
    """two thirds noisy copies of library rows (a spread of high scores), one third unrelated; at most
    45 + 18 non-zeros, so every query also has an entry list (64 entries)"""
    q = _rows(rng, nq, 8, 18)
    for i in range(2 * nq // 3):
        v = x[rng.integers(len(x))].copy()
        v[rng.random(DIM) < 0.3] = 0.0
        v += 0.2 * q[i]
        q[i] = v / np.linalg.norm(v)
    return q


def _host_ivf(O, idx):
    """the oracle's view of what the index stores: same centroids, codebooks, lists and codes"""
    off, ids, payload = idx.lists()
    info = idx.info()
    ivf = O.HostIVF.__new__(O.HostIVF)
    ivf.centroids, ivf.nlist, ivf.d = idx.centroids(), info.nlist, info.d
    ivf.list_offsets, ivf.ids, ivf.payload, ivf.codebooks = off, ids, payload, idx.codebooks()
    ivf.kind = 1
    return ivf


def _filtered(O, ivf, keep_by_id):
    """The oracle's IVF with only the vectors whose id is kept (same lists, same order inside a list)."""
    keep = keep_by_id[ivf.ids]
    lst = np.repeat(np.arange(ivf.nlist), np.diff(ivf.list_offsets))
    out = O.HostIVF.__new__(O.HostIVF)
    out.centroids, out.nlist, out.d, out.codebooks, out.kind = ivf.centroids, ivf.nlist, ivf.d, ivf.codebooks, 1
    out.list_offsets = np.concatenate([[0], np.cumsum(np.bincount(lst[keep], minlength=ivf.nlist))]).astype(np.int32)
    out.ids = np.ascontiguousarray(ivf.ids[keep])
    out.payload = np.ascontiguousarray(ivf.payload[keep])
    return out


def _make(cen, cb, x):
    from ann_solo_amd import faiss_compat as faiss
    idx = faiss.IndexIVFPQ(faiss.IndexFlatIP(DIM), DIM, len(cen), 32, 8)
    idx.set_trained(cen, cb)
    idx.add(x)
    return idx


def _same_rows(D, I, Do, Io, what):
    assert np.array_equal(I, Io), what
    assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)), what


def _same_sets(Du, Iu, Do, Io, what):
    """unordered rows: the oracle's ids with the oracle's score bits, padding last"""
    for r in range(len(Io)):
        n = int((Io[r] >= 0).sum())
        assert (Iu[r, :n] >= 0).all() and (Iu[r, n:] == -1).all(), (what, r)
        o, ou = np.argsort(Io[r, :n]), np.argsort(Iu[r, :n])
        assert np.array_equal(Io[r, :n][o], Iu[r, :n][ou]), (what, r)
        assert np.array_equal(Do[r, :n][o].view(np.uint32), Du[r, :n][ou].view(np.uint32)), (what, r)


def _unpack(K):
    """packed rows -> (ids, -1 = empty; score bits)"""
    K = np.asarray(K).view(np.uint64)
    ids = np.where(K != 0, 0xFFFFFFFF - (K & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    ordb = (K >> np.uint64(32)).astype(np.uint32)
    bits = np.where(ordb & 0x80000000, ordb & 0x7fffffff, ~ordb).astype(np.uint32)   # ord2f
    return ids, bits


def _same_keys(K, Do, Io, what):
    ids, bits = _unpack(K)
    for r in range(len(Io)):
        n = int((Io[r] >= 0).sum())
        assert (ids[r] >= 0).sum() == n, (what, r)
        o, ok = np.argsort(Io[r, :n]), np.argsort(np.where(ids[r] >= 0, ids[r], 1 << 40))[:n]
        assert np.array_equal(Io[r, :n][o], ids[r][ok]), (what, r)
        assert np.array_equal(Do[r, :n][o].view(np.uint32), bits[r][ok]), (what, r)


def _window_mask(q_pmz, key, charge, tol):
    """precursor_ok (csrc/common.hpp), Da mode, over a key column, in the same double arithmetic"""
    return np.abs(q_pmz - np.asarray(key, np.float32).astype(np.float64)) * float(charge) <= tol


@pytest.fixture(scope='module')
def world(O):
    """One trained quantiser pair (GPU training, read back: the oracle searches the same codes), the
    library vectors and the queries."""
    from ann_solo_amd import faiss_compat as faiss
    rng = np.random.default_rng(2024)
    x = _rows(rng, N)
    xq = _queries(rng, x, NQ)
    idx = faiss.IndexIVFPQ(faiss.IndexFlatIP(DIM), DIM, NLIST, 32, 8)
    idx.set_niter(4)
    idx.train(x[:8000])
    idx.add(x)
    return dict(x=x, xq=xq, idx=idx, ivf=_host_ivf(O, idx), cen=idx.centroids(), cb=idx.codebooks(), rng=rng)


@pytest.mark.parametrize('k,nprobe', [(1280, NLIST), (2048, NLIST), (1024, NLIST), (1, NLIST), (1280, 1), (2048, 2),
                                      (1024, 7)])
def test_sorted_and_set_rows(world, k, nprobe):
    """k = 1280 / 2048 leave the 2048- / 4096-key buffer its smallest slack (many syncs per query, over
    two table chunks at nprobe = nlist); k = 1 syncs once; one or two lists hold fewer than k vectors."""
    idx, ivf, xq = world['idx'], world['ivf'], world['xq']
    idx.nprobe = nprobe
    Do, Io = ivf.search(xq, k, nprobe)
    if nprobe <= 2:
        assert (Io == -1).any()
    D, I = idx.search(xq, k)
    _same_rows(D, I, Do, Io, (k, nprobe))
    idx.set_unordered(True)
    try:
        Du, Iu = idx.search(xq, k)
    finally:
        idx.set_unordered(False)
    _same_sets(Du, Iu, Do, Io, (k, nprobe))


@pytest.mark.parametrize('k', [1024, 1280, 2048])
def test_bit_identical_scores_fall_back_to_exact_flushes(O, world, k):
    """Five distinct vectors, 4000 copies each: thousands of equal scores in the threshold bucket, which
    no compaction can thin out -- the top-k switches to sort-and-truncate flushes behind the
    free-running appends, and ties are ranked by id."""
    rng = np.random.default_rng(7)
    base = _rows(rng, 5)
    x = np.concatenate([np.repeat(base, 4000, axis=0), _rows(rng, 2000)])
    x = x[rng.permutation(len(x))]
    xq = np.concatenate([base, _queries(rng, x, 11)])
    idx = _make(world['cen'], world['cb'], x)
    ivf = _host_ivf(O, idx)
    idx.nprobe = NLIST
    Do, Io = ivf.search(xq, k, NLIST)
    assert all(len(np.unique(Do[r])) < k // 8 for r in range(5))      # the rows of the copies are ties
    D, I = idx.search(xq, k)
    _same_rows(D, I, Do, Io, k)
    idx.set_unordered(True)
    try:
        Du, Iu = idx.search(xq, k)
    finally:
        idx.set_unordered(False)
    _same_sets(Du, Iu, Do, Io, k)


def test_more_than_512_probes_and_its_window_scan(O, world):
    """nprobe > 512: two probes per thread, with both key buffers; and the window scan of the same index."""
    rng = np.random.default_rng(11)
    nlist = 600
    x, xq = world['x'], world['xq']
    idx = _make(_rows(rng, nlist), world['cb'], x)
    ivf = _host_ivf(O, idx)
    idx.nprobe = nlist
    for k in (1280, 2048):
        Do, Io = ivf.search(xq, k, nlist)
        D, I = idx.search(xq, k)
        _same_rows(D, I, Do, Io, k)
    key = rng.uniform(400.0, 1400.0, len(x)).astype(np.float32)
    q_pmz = rng.uniform(500.0, 1300.0, len(xq))
    idx.set_window_key(key)
    D, I = idx.search_window(xq, 1280, q_pmz, 2, 300.0, 'Da')
    for i in range(len(xq)):
        keep = _window_mask(q_pmz[i], key, 2, 300.0)
        rD, rI = _filtered(O, ivf, keep).search(xq[i:i + 1], 1280, nlist)
        _same_rows(D[i:i + 1], I[i:i + 1], rD, rI, i)


@pytest.mark.parametrize('k,tol', [(1280, 300.0), (1024, 1e9), (1280, 40.0)])
def test_window_scan(O, world, k, tol):
    """asl_index_search_window: the runs of the window-ordered lists, first and last tile partly in
    (12-byte table entries, 168 per chunk); a narrow window leaves fewer than k vectors."""
    idx, ivf, xq = world['idx'], world['ivf'], world['xq']
    rng = np.random.default_rng(13)
    key = rng.uniform(400.0, 1400.0, N).astype(np.float32)
    q_pmz = rng.uniform(500.0, 1300.0, len(xq))
    idx.nprobe = NLIST
    idx.set_window_key(key)
    D, I = idx.search_window(xq, k, q_pmz, 2, tol, 'Da')
    for i in range(len(xq)):
        keep = _window_mask(q_pmz[i], key, 2, tol)
        rD, rI = _filtered(O, ivf, keep).search(xq[i:i + 1], k, NLIST)
        _same_rows(D[i:i + 1], I[i:i + 1], rD, rI, (tol, i))
    if tol == 40.0:
        assert (I == -1).any()


def test_packed_key_rows_of_three_shards_merge_to_the_oracle(world):
    """set_mode 2: rows of packed (score, ~id) keys, one per shard, merged by asl_topk_merge_keys"""
    from ann_solo_amd import faiss_compat as faiss
    idx, ivf, x, xq = world['idx'], world['ivf'], world['x'], world['xq']
    k = 1280
    Do, Io = ivf.search(xq, k, NLIST)
    cD, cI = idx.coarse(xq, NLIST)
    _same_keys(idx.search_preassigned_keys(xq, k, cD, cI), Do, Io, 'unsharded')
    parts = []
    for r in range(3):
        sh = _make(world['cen'], world['cb'], x)
        sh.shard(r, 3)
        parts.append(sh.search_preassigned_keys(xq, k, cD, cI))
    Dm, Im = faiss.topk_merge_keys(np.stack(parts))
    _same_rows(Dm, Im, Do, Io, 'merged')


def test_gated_launch_on_a_shard(O, world):
    """asl_index_search_entries with a device-side row count (the shard-side rescans of the sharded
    search): the first `count` rows equal the oracle's search over the shard's own lists."""
    x, xq = world['x'], world['xq']
    sh = _make(world['cen'], world['cb'], x)
    sh.shard(1, 3)
    ivf = _host_ivf(O, sh)
    assert 0 < len(ivf.ids) < len(x)
    k = 1024
    Do, Io = ivf.search(xq, k, NLIST)
    ent = np.zeros((len(xq), 64, 2), np.int32)
    cnt = np.zeros(len(xq), np.int32)
    for i in range(len(xq)):
        nz = np.nonzero(xq[i])[0]
        assert len(nz) <= 64
        cnt[i] = len(nz)
        ent[i, :len(nz), 0] = nz * 128
        ent[i, :len(nz), 1] = xq[i, nz].view(np.int32)
    cD, cI = world['idx'].coarse(torch.from_numpy(xq).cuda(), NLIST)
    ent_d, cnt_d = torch.from_numpy(ent).cuda(), torch.from_numpy(cnt).cuda()
    for count in (len(xq), 9, 0):
        gate = torch.tensor([count], dtype=torch.int32, device='cuda')
        K = sh.search_entries_keys(ent_d, cnt_d, k, cD, cI, gate=gate)
        torch.cuda.synchronize()
        _same_keys(K[:count].cpu().numpy(), Do[:count], Io[:count], count)


@pytest.mark.parametrize('k', [1280, 2048])
def test_chunk_boundary_with_holes_in_the_probe_list(O, world, k):
    """More than 256 tiles per query, a probe list with -1 entries and lists that are empty: the waves
    finish their shares of a chunk at different times and keep answering the syncs of the others."""
    rng = np.random.default_rng(17)
    x, xq = world['x'], world['xq']
    cen = np.concatenate([world['cen'], -_rows(rng, 6)])      # six centroids no vector is assigned to
    cen = cen[rng.permutation(len(cen))]
    nlist = len(cen)
    idx = _make(cen, world['cb'], x)
    ivf = _host_ivf(O, idx)
    sizes = np.diff(ivf.list_offsets)
    assert (sizes == 0).sum() >= 6 and sizes.sum() == N
    cD, cI = idx.coarse(xq, nlist)
    assert cI.shape[1] == nlist
    dropped = np.argsort(sizes)[[8, 15, 22, 29, 40]]           # lists of several sizes leave the probe lists
    cI = np.where(np.isin(cI, dropped), -1, cI).astype(np.int32)
    assert (cI == -1).sum() == 5 * len(xq)
    lst = np.repeat(np.arange(nlist), sizes)
    keep = np.ones(N, bool)
    keep[ivf.ids[np.isin(lst, dropped)]] = False
    assert keep.sum() > 256 * 64
    Do, Io = _filtered(O, ivf, keep).search(xq, k, nlist)
    D, I = idx.search_preassigned(xq, k, cD, cI)
    _same_rows(D, I, Do, Io, k)
