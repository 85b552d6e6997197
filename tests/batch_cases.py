"""Batch-shape cases of the per-query entry points (a helper, not a test): small POOLS of items and
the BATCHES gathered from them. The answer for a query must not depend on its neighbours, its position
or the batch size, while much of the host and kernel code decides what to do from the batch: the coarse
quantiser's gate, the row chunks behind the 1 GiB score workspace, the rescoring's list split, the
spectra per workgroup of the encoder. tests/test_gpu_batch_shapes.py computes every item's expectation
once, with the oracle, and compares every row of every batch with it as bits;
tests/test_batch_cases_cpu.py shows that the cases reach the decisions they are meant to reach.

numpy only (and, where a builder says so, the oracle handed in): nothing here touches the GPU. Batches
are drawn from seeded generators WITH replacement, so an item meets different neighbours and positions
and sometimes itself."""
import numpy as np

# ------------------------------------------------------------------ 1. coarse scores under every gate outcome
COARSE_D = 800
COARSE_NLISTS = (256, 33)      # float4 tile loads and full tiles | scalar loads, a partial tile, odd ld
COARSE_CAP = 64                # entries a row keeps in registers (coarse_sparse.hip: CS_CAP); more: a dense row
# (m, number of dense rows)
COARSE_CASES = ((1, 0), (1, 1), (2, 1), (3, 0), (4, 0), (5, 0), (63, 0), (63, 1),
                (64, 0), (64, 1), (64, 2), (65, 1),
                (127, 1), (127, 2), (128, 2), (128, 3), (129, 2), (129, 3), (257, 4), (257, 5))


def gemm_takes_the_batch(m, n_over):
    """The gate: index_search.hip:26 `over_max = m / 64`, coarse_sparse.hip:112 `if (*n_over > over_max) return;`
    (and the GEMM gated the other way on the same counter)."""
    return n_over > m // 64


def sparse_rows(rng, n, d, nnz_lo, nnz_hi, neg=0.0):
    """n unit rows of nnz_lo .. nnz_hi non-zeros (a count of 0 gives the all-zero row); a fraction `neg`
    of the components negative."""
    x = np.zeros((n, d), np.float32)
    for i in range(n):
        k = int(rng.integers(nnz_lo, nnz_hi + 1))
        c = rng.choice(d, size=min(k, d), replace=False)
        v = (rng.random(len(c)) + 0.05).astype(np.float32)
        x[i, c] = np.where(rng.random(len(c)) < neg, -v, v)
    return (x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-20)).astype(np.float32)


def coarse_centroids(nlist, d=COARSE_D):
    """As tests/test_gpu_index.py's sparse coarse test: 8 .. 200 non-zeros, signed."""
    rng = np.random.default_rng(7000 + nlist)
    cen = sparse_rows(rng, nlist, d, 8, min(d, 200), neg=0.25)
    cen[1] *= -1.0
    return cen


def coarse_pool(d=COARSE_D):
    """96 rows: 72 of 0 .. 50 non-zeros (row 0 is all-zero), 8 of exactly 64 (the most a row keeps in
    registers), 16 of 65 .. 90 (dense rows: the ones the gate counts). Returns (rows, dense mask)."""
    rng = np.random.default_rng(7100 + d)
    x = np.concatenate([sparse_rows(rng, 1, d, 0, 0), sparse_rows(rng, 71, d, 0, 50, neg=0.2),
                        sparse_rows(rng, 8, d, 64, 64, neg=0.2), sparse_rows(rng, 16, d, 65, 90, neg=0.2)])
    return x, np.count_nonzero(x, axis=1) > COARSE_CAP


def dense_positions(m, n_dense, turn):
    """Where a batch of m rows holds its dense rows: first, last and middle in turn, then the quarters."""
    spots = [0, m - 1, m // 2, m // 4, (3 * m) // 4, m // 8, (7 * m) // 8]
    spots = spots[turn % 3:] + spots[:turn % 3]
    out = []
    for s in spots:
        if s not in out and len(out) < n_dense:
            out.append(s)
    assert len(out) == n_dense, (m, n_dense)
    return out


def coarse_batches(dense_mask):
    """[(m, n_dense, pool rows [m])] for COARSE_CASES: the dense rows where dense_positions puts them, every
    other row drawn with replacement from the rows that are not dense."""
    rng = np.random.default_rng(7200)
    dense, plain = np.nonzero(dense_mask)[0], np.nonzero(~dense_mask)[0]
    out = []
    for turn, (m, n_dense) in enumerate(COARSE_CASES):
        take = rng.choice(plain, m)
        for s in dense_positions(m, n_dense, turn):
            take[s] = rng.choice(dense)
        out.append((m, n_dense, take))
    return out


# ------------------------------------------------------------------ 2. index search at odd batch sizes
INDEX_N, INDEX_NLIST, INDEX_NITER, INDEX_K, INDEX_NPROBE = 5000, 16, 4, 100, 8
INDEX_KINDS = ('flat', 'ivfflat_fp32', 'ivfflat_fx22', 'ivfpq')
INDEX_SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257)
INDEX_SPARSE, INDEX_DENSE = 64, 8
ENC = dict(min_bound=10.96, bin_size=0.04, hash_len=800)


def _encode(O, pack):
    o, mz, inten, *_ = pack
    return O.encode_batch(mz, inten, o, ENC['min_bound'], ENC['bin_size'], ENC['hash_len'])


def many_peak_spectra(rng, n, lo=70, hi=90):
    """(offsets, mz, intensity) of n spectra of lo .. hi peaks at distinct m/z."""
    off, mzs, its = [0], [], []
    for _ in range(n):
        k = int(rng.integers(lo, hi + 1))
        mzs.append(np.sort(rng.uniform(100.0, 1900.0, k)).astype(np.float32))
        its.append((rng.random(k) + 0.05).astype(np.float32))
        off.append(off[-1] + k)
    return np.asarray(off, np.int32), np.concatenate(mzs), np.concatenate(its)


def index_vectors(O):
    """(xb [5000, 800], pool [72, 800], dense mask): the encoded library, 64 encoded queries of it and 8 rows
    encoded from spectra of 70 .. 90 peaks with more than 64 non-zeros (redrawn until they have them)."""
    from ann_solo_amd import synthetic
    lib, aux = synthetic.make_library(INDEX_N, seed=7300, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, INDEX_SPARSE, seed=7301, charge=2)
    xb, sparse = _encode(O, lib.numpy()), _encode(O, q.numpy())
    rng = np.random.default_rng(7302)
    dense = np.zeros((0, ENC['hash_len']), np.float32)
    while len(dense) < INDEX_DENSE:
        o, mz, inten = many_peak_spectra(rng, INDEX_DENSE)
        v = O.encode_batch(mz, inten, o, ENC['min_bound'], ENC['bin_size'], ENC['hash_len'])
        dense = np.concatenate([dense, v[np.count_nonzero(v, axis=1) > COARSE_CAP]])[:INDEX_DENSE]
    pool = np.ascontiguousarray(np.concatenate([sparse, dense]))
    return xb, pool, np.count_nonzero(pool, axis=1) > COARSE_CAP


def index_batches(dense_mask):
    """[(size, draw, pool rows)]: two draws per size. Draw 0 is uniform over the whole pool (from 63 rows on it
    holds a dense row, one is put in if the draw has none): so many dense rows that the gate hands the batch to
    the GEMM. Draw 1 takes sparse rows and exactly size // 64 dense ones: the most the sparse kernel keeps."""
    rng = np.random.default_rng(7400)
    dense, plain = np.nonzero(dense_mask)[0], np.nonzero(~dense_mask)[0]
    out = []
    for size in INDEX_SIZES:
        take = rng.integers(0, len(dense_mask), size)
        if size >= 63 and not dense_mask[take].any():
            take[int(rng.integers(0, size))] = rng.choice(dense)
        out.append((size, 0, take))
        take = rng.choice(plain, size)
        for s in rng.choice(size, size // 64, replace=False):
            take[s] = rng.choice(dense)
        out.append((size, 1, take))
    return out


# ------------------------------------------------------------------ 3. the chunk loops at 1 GiB
SCORE_CHUNK_BYTES = 1 << 30        # index.hpp
CHUNK_POOL = 37                    # coprime with every chunk height below: a row that reads another chunk's
                                   # bitmap, bound or output slot reads another item's
CHUNK_N, CHUNK_D = 1 << 18, 4      # a score row of 1 MiB: 1024 rows per chunk
CHUNK_FLAT = ((1025, 10), (2049, 10), (1025, 2058))      # (nq, k) on IndexFlatIP; k = 2058: the bounded second pass
CHUNK_IVF = dict(nlist=33, nprobe=5, nq=1025, k=10)      # IVF-Flat, scan variant 1: GEMM plus probe bitmap
CLOOP = dict(nlist=4096, d=64, nnz=4, n=8192, nq=65537, nprobe=16, k=10)     # the coarse quantiser's own loop


def chunk_rows(ncol):
    """Rows per chunk of a score matrix with ncol columns (index_search.hip: coarse_search, search_gemm_topk)."""
    return max(1, SCORE_CHUNK_BYTES // (ncol * 4))


def periodic(pool, nq):
    """Row r is pool[r % len(pool)]."""
    return np.ascontiguousarray(pool[np.arange(nq) % len(pool)])


def chunk_vectors():
    """(xb [2^18, 4], pool [37, 4]) random normal."""
    rng = np.random.default_rng(7500)
    return (rng.standard_normal((CHUNK_N, CHUNK_D)).astype(np.float32),
            rng.standard_normal((CHUNK_POOL, CHUNK_D)).astype(np.float32))


def signed_sparse(rng, n, d, nnz):
    x = np.zeros((n, d), np.float32)
    for i in range(n):
        x[i, rng.choice(d, nnz, replace=False)] = rng.standard_normal(nnz).astype(np.float32)
    return x


def cloop_vectors():
    """(centroids [4096, 64], xb [8192, 64], pool [37, 64]), 4 non-zeros a row."""
    rng = np.random.default_rng(7600)
    c = CLOOP
    return tuple(signed_sparse(rng, n, c['d'], c['nnz']) for n in (c['nlist'], c['n'], CHUNK_POOL))


# ------------------------------------------------------------------ 4. rescoring with split lists
RS_TOL = 0.02
RS_NLIB, RS_NPOOL = 64, 4
# (nq, list lengths); `None`: every list of RS_LONG slots, the queries periodic over the pool
RS_LONG = 4097
RS_CASES = ((1, [4096]), (1, [4097]), (1, [8193]), (1, [258049]), (1, [300000]),
            (2, [8192, 0]), (2, [8194, 0]), (3, [12289, 1, 1]), (2047, None), (2048, None))
RS_YSPLIT = (1, 2, 3, 64, 64, 1, 2, 2, 2, 1)       # what each case is meant to reach
RS_TOL0_CASES = (0, 1, 2)                          # ... also at tol = 0.0
RS_TOPN_CASES = (0, 1, 2, 5, 6, 7)                 # the small ones: also ranked, n_best = 3


def ysplit(nq, total_slots):
    """rescore.hip, rescore_device: `avg = total_slots / nq; if (nq < 2048 && avg > 4096) ysplit = min(64, cdiv(avg, 4096))`."""
    avg = total_slots // max(nq, 1)
    return min(64, -(-avg // 4096)) if nq < 2048 and avg > 4096 else 1


def _pack(spectra, pmz, pz):
    off = np.concatenate([[0], np.cumsum([len(s[0]) for s in spectra])]).astype(np.int64)
    cat = lambda i, dt: np.concatenate([s[i] for s in spectra]).astype(dt)
    return (off, cat(0, np.float32), cat(1, np.float32), cat(2, np.uint8), np.asarray(pmz, np.float64),
            np.asarray(pz, np.int64))


def rescore_spectra():
    """(library, pool), six packed arrays each. Every m/z comes from one grid of 400 float32 values at least
    0.2 apart, so spectra share peaks exactly (scores are positive at tol = 0 too). Library rows 0 .. 39: 20 .. 64
    peaks; 40 .. 51: 65 .. 150 peaks (the binary-search kernel; row 45 has 120); 52 .. 63: 30 .. 60 peaks, one
    of them with a twin half a tolerance above it (a doubly matched peak: the pair kernel). Pool: query 0 holds
    the peaks of row 5, query 1 those of twin row 55, query 2 those of row 45 (more than 100 peaks: the whole
    query goes to the binary-search kernel), query 3 those of twin row 58 and of row 10 -- each with other
    intensities and a few grid peaks more."""
    rng = np.random.default_rng(7700)
    grid = (100.0 + np.cumsum(rng.uniform(0.2, 8.0, 400))).astype(np.float32)
    assert grid[-1] < 1950.0

    def inten(n):
        it = rng.lognormal(0, 1, n).astype(np.float32)
        return (it / np.float32(np.linalg.norm(it))).astype(np.float32)

    def spectrum(at, twin_of=None):
        mz = grid[np.sort(at)]
        if twin_of is not None:
            mz = np.sort(np.concatenate([mz, [np.float32(grid[twin_of] + np.float32(RS_TOL / 2))]])).astype(np.float32)
        return mz, inten(len(mz)), rng.integers(0, 3, len(mz)).astype(np.uint8)

    picks, twins, lib = [], {}, []
    for r in range(RS_NLIB):
        n = 120 if r == 45 else int(rng.integers(65, 151)) if 40 <= r < 52 else \
            int(rng.integers(30, 61)) if r >= 52 else int(rng.integers(20, 65))
        at = rng.choice(len(grid), n, replace=False)
        picks.append(at)
        if r >= 52:
            twins[r] = int(at[0])
        lib.append(spectrum(at, twins.get(r)))
    pool = []
    for base, extra in (((5,), 10), ((55,), 8), ((45,), 5), ((58, 10), 4)):
        at = np.unique(np.concatenate([picks[b] for b in base] + [rng.choice(len(grid), extra, replace=False)]))
        pool.append(spectrum(at))
    return (_pack(lib, rng.uniform(400, 900, RS_NLIB), np.full(RS_NLIB, 2)),
            _pack(pool, rng.uniform(400, 900, RS_NPOOL), np.full(RS_NPOOL, 2)))


def rescore_case(index, S):
    """(pool item of every query [nq], candidate rows, offsets [nq + 1]) of RS_CASES[index]; S [pool, library]:
    the exact scores, which say where the constructed list puts its winner. Lists are drawn with replacement
    (rows repeat). Where the lists are split, query 0's list holds its best row at slot 40, again at slot
    64 * ysplit + 3 and at the end, and lower-scoring rows everywhere else: groups of 32 slots go to the blocks
    round robin, so another block meets the winner earlier than block 0 does, and position 40 has to win."""
    nq, lens = RS_CASES[index]
    lens = [RS_LONG] * nq if lens is None else lens
    rng = np.random.default_rng(7800 + index)
    item = np.arange(nq) % RS_NPOOL
    lists = [rng.integers(0, RS_NLIB, n).astype(np.int64) for n in lens]
    ys = ysplit(nq, sum(lens))
    if ys > 1:
        w = int(np.argmax(S[item[0]]))
        lower = np.nonzero(S[item[0]] < S[item[0], w])[0]
        lists[0] = rng.choice(lower, lens[0]).astype(np.int64)
        lists[0][[40, 64 * ys + 3, lens[0] - 1]] = w
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return item, np.concatenate(lists), off


def gather_spectra(pack, items):
    """The packed arrays of pack's spectra `items`, in that order."""
    o, mz, it, chg, pmz, pz = pack
    sl = [slice(o[i], o[i + 1]) for i in items]
    return _pack([(mz[s], it[s], chg[s]) for s in sl], pmz[items], pz[items])


# ------------------------------------------------------------------ 5. encoder
ENC_SIZES = (0, 1, 2, 63, 64, 65, 200)     # peaks of the first pool spectra; the others: 1 .. 90
ENC_POOL = 24
ENC_BATCHES = (1, 2, 3, 4, 5, 7, 8, 9)     # around ENC_WAVES = 4 spectra per workgroup (encode.hip)


def encoder_pool():
    """(offsets, mz, intensity) of 24 spectra with colliding bins: about three peaks per distinct m/z (the
    long ones mostly distinct: more than 64 non-zeros), intensities of very different magnitude."""
    rng = np.random.default_rng(7900)
    off, mzs, its = [0], [], []
    for npk in list(ENC_SIZES) + list(rng.integers(1, 91, ENC_POOL - len(ENC_SIZES))):
        npk = int(npk)
        base = rng.uniform(100, 1900, max(1, npk if npk > 100 else npk // 3 + 1)).astype(np.float32)
        mzs.append(base[rng.integers(0, len(base), npk)])
        its.append((rng.random(npk) * 10.0 ** rng.integers(-6, 4, npk)).astype(np.float32))
        off.append(off[-1] + npk)
    return np.asarray(off, np.int32), np.concatenate(mzs).astype(np.float32), np.concatenate(its).astype(np.float32)


def encoder_batches():
    """[pool items]: three draws with replacement per batch size."""
    rng = np.random.default_rng(7901)
    return [rng.integers(0, ENC_POOL, n) for n in ENC_BATCHES for _ in range(3)]


def gather_peaks(pool, items):
    o, mz, it = pool
    sl = [slice(o[i], o[i + 1]) for i in items]
    off = np.concatenate([[0], np.cumsum([o[i + 1] - o[i] for i in items])]).astype(np.int32)
    cat = lambda a: np.concatenate([a[s] for s in sl]).astype(np.float32) if len(sl) else np.zeros(0, np.float32)
    return off, cat(mz), cat(it)


FUSED_SIZES = (1, 3, 65, 129)
