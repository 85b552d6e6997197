"""The reference of the per-query interval window (ASL_TOL_INTERVAL) -- a helper, not a test. The
reference is the unchanged oracle: for query i the key column becomes ``key_i = where(lo_i <= key <= hi_i,
key, NaN)`` (float64 comparison of the promoted float32 column) and the oracle's own Da test runs on
``key_i`` with tol = 1e30, so a row passes iff its key is not NaN. 'post' order: the oracle's batch over the
unfiltered index with ``key_i``; 'pre' order and the index level: over the index filtered to ``key_i``'s
finite rows (the ``_filtered`` construction of the window-scan tests). numpy and the oracle only; the shapes
are those of the window-scan tests (the 5 000-spectrum tie library)."""
import numpy as np

TOL_ALL = 1e30          # the oracle's Da test with this tolerance passes every finite key
CHARGE = 2
FRAG_TOL = 0.02
NEG_MAX = np.float32(-3.4028234663852886e38)


# ------------------------------------------------------------------ the rule
def interval_mask(key, lo, hi):
    """The direct definition: lo <= (double)key && (double)key <= hi; NaN (key or bound) never passes."""
    l = np.asarray(key, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore'):
        return (np.float64(lo) <= l) & (l <= np.float64(hi))


def masked_key(key, lo, hi):
    """key_i: the float32 key where the row passes query i's interval, NaN elsewhere."""
    key = np.asarray(key, np.float32)
    return np.where(interval_mask(key, lo, hi), key, np.float32(np.nan)).astype(np.float32)


def oracle_passes(O, key_i, q_pmz=500.0):
    """What the oracle's own window test (Da, tol 1e30) keeps of key_i."""
    return np.array([O.precursor_ok(q_pmz, v, CHARGE, TOL_ALL, 'Da') for v in key_i], bool)


def derived(q_pmz, charge, lo_da, hi_da):
    """Intervals of library m/z for a signed range of the neutral mass difference (query - library) * charge."""
    q = np.asarray(q_pmz, np.float64)
    return np.stack([q - np.float64(hi_da) / charge, q - np.float64(lo_da) / charge], axis=1)


def window_cases(q_pmz, key, copies):
    """name -> [nq, 2] float64: the windows the tests cover. ``copies``: the first queries are copies of
    library row 0 (precursor m/z of row 0 + 7)."""
    q = np.asarray(q_pmz, np.float64)
    key = np.asarray(key, np.float32)
    nq = len(q)
    out = {
        'm50_p250': derived(q, CHARGE, -50.0, 250.0),
        'p10_p250': derived(q, CHARGE, 10.0, 250.0),           # excludes the unmodified match
        'm250_m10': derived(q, CHARGE, -250.0, -10.0),
        'iso4': np.stack([q - 1.0, q + 3.0], axis=1),          # a 4 m/z isolation window, not centred
        'empty': np.stack([q + 1.0, q - 1.0], axis=1),         # lo > hi
        'all': np.tile(np.array([-np.inf, np.inf]), (nq, 1)),
    }
    # exactly one library row: that row's own float32 key as both bounds (rows with a unique key; the
    # copies of row 0 take rows of the tie block)
    uniq, cnt = np.unique(key[np.isfinite(key)], return_counts=True)
    single = set(uniq[cnt == 1].tolist())
    rows = []
    for i in range(nq):
        r = (i * 53) % 400 if i < copies else (400 + i * 37) % len(key)
        while float(key[r]) not in single:
            r = (r + 1) % len(key)
        rows.append(r)
    one = key[rows].astype(np.float64)
    out['one_row'] = np.stack([one, one], axis=1)
    nan = out['m50_p250'].copy()
    nan[::5, 0] = np.nan
    nan[3::7, 1] = np.nan
    out['nan_some'] = nan
    return out, np.asarray(rows)


# ------------------------------------------------------------------ the oracle's index
def host_ivf(O, idx):
    """``O.HostIVF`` over what the index holds (``idx.lists()``): IVF-PQ codes or IVF-Flat vectors."""
    off, ids, payload = idx.lists()
    info = idx.info()
    ivf = O.HostIVF.__new__(O.HostIVF)
    ivf.centroids, ivf.nlist, ivf.d = idx.centroids(), info.nlist, info.d
    ivf.list_offsets, ivf.ids, ivf.payload = off, ids, payload
    pq = payload.dtype == np.uint8
    ivf.codebooks = idx.codebooks() if pq else None
    ivf.kind = 1 if pq else 0
    return ivf


def filtered(O, ivf, keep_by_id):
    """The oracle's IVF with only the vectors whose id is kept: same lists, same order inside a list."""
    keep_by_id = np.asarray(keep_by_id, bool)
    keep = keep_by_id[ivf.ids]
    lst = np.repeat(np.arange(ivf.nlist), np.diff(ivf.list_offsets))
    out = O.HostIVF.__new__(O.HostIVF)
    out.centroids, out.nlist, out.d, out.kind = ivf.centroids, ivf.nlist, ivf.d, ivf.kind
    out.codebooks = getattr(ivf, 'codebooks', None)
    out.list_offsets = np.concatenate([[0], np.cumsum(np.bincount(lst[keep], minlength=ivf.nlist))]).astype(np.int32)
    out.ids = np.ascontiguousarray(ivf.ids[keep])
    out.payload = np.ascontiguousarray(ivf.payload[keep])
    return out


def index_rows(O, ivf, xq, k, nprobe, key, wins):
    """(D, I) [nq, k] of the index level: per query the oracle's search over the index filtered to the finite
    rows of key_i."""
    D = np.full((len(xq), k), NEG_MAX, np.float32)
    I = np.full((len(xq), k), -1, np.int64)
    for i in range(len(xq)):
        keep = np.isfinite(masked_key(key, wins[i, 0], wins[i, 1]))
        D[i], I[i] = (a[0] for a in filtered(O, ivf, keep).search(xq[i:i + 1], k, nprobe))
    return D, I


def assert_rows_equal(got, want, what=''):
    """ids equal; where a row holds a hit, score bits equal; beyond the hits -1 and -FLT_MAX."""
    (D, I), (rD, rI) = got, want
    D, I = np.asarray(D), np.asarray(I)
    assert np.array_equal(I, rI), what
    v = rI >= 0
    assert np.array_equal(D[v].view(np.uint32), np.asarray(rD)[v].view(np.uint32)), what
    assert (D[~v] == NEG_MAX).all(), what


# ------------------------------------------------------------------ the oracle's batch
def spectra_rows(O, q, rows):
    o, mz, it, chg, pmz, pz = q.numpy()
    sel = [(int(o[i]), int(o[i + 1])) for i in rows]
    offs = np.concatenate([[0], np.cumsum([e - s for s, e in sel])]).astype(np.int32)
    cat = lambda a: np.concatenate([a[s:e] for s, e in sel])
    return O.Spectra(offs, cat(mz), cat(it), cat(chg), pmz[list(rows)], pz[list(rows)])


def oracle_batch(O, q, L, ivf, key, wins, k, nprobe, order, stride=64):
    """The oracle's fused batch, query by query (every query has a key column of its own): dict of best_row,
    best_score, n_cand, pm_count, pm_pairs, knn_I. order 'post': top-k of the probed lists, then the window;
    'pre': the k best in-window vectors of the probed lists."""
    rows = []
    for i in range(q.n):
        key_i = masked_key(key, wins[i, 0], wins[i, 1])
        use = ivf if order == 'post' else filtered(O, ivf, np.isfinite(key_i))
        rows.append(O.search_batch(spectra_rows(O, q, [i]), L, key_i, CHARGE, use, k, nprobe, TOL_ALL, 'Da',
                                   FRAG_TOL, True, pm_stride=stride, want_knn=True))
    return {f: np.concatenate([r[f] for r in rows]) for f in rows[0]}


def window_rows(key, wins, i):
    """The candidates of a window-only search (use_ann = 0): the finite rows of key_i, ascending."""
    return np.nonzero(np.isfinite(masked_key(key, wins[i, 0], wins[i, 1])))[0].astype(np.int64)


def oracle_ranks(O, Q, i, L, cand, n, groups=None):
    """[(row, score, matches)]: O.best_match, the winner deleted, until n ranks (of n different groups);
    equal scores go to the lower library row."""
    cand = np.sort(np.asarray(cand, np.int64))
    out, seen = [], set()
    while len(out) < n and len(cand):
        b, s, m = O.best_match(Q, i, L, cand, FRAG_TOL, True)
        if b < 0:
            break
        row = int(cand[b])
        cand = np.delete(cand, b)
        if groups is not None and int(groups[row]) >= 0:
            if int(groups[row]) in seen:
                continue
            seen.add(int(groups[row]))
        out.append((row, s, m))
    return out


# ------------------------------------------------------------------ the shapes (the window-scan tests')
def tie_library(n=5000, seed=71):
    """synthetic library whose rows 0 .. 399 are copies of row 0 spread over +-300 Da (score ties)."""
    from ann_solo_amd import synthetic
    from ann_solo_amd.packed import PackedSpectra
    lib0, aux = synthetic.make_library(n, seed=seed, device='cpu', charges=(2,), charge_p=(1.0,))
    o, mz, it, chg, pmz, pz = lib0.numpy()
    a, b = int(o[0]), int(o[1])
    rng = np.random.default_rng(5)
    offs = [0]
    MZ, IT, CH, PM = [], [], [], []
    for r in range(lib0.n):
        s, e = (a, b) if r < 400 else (int(o[r]), int(o[r + 1]))
        MZ.append(mz[s:e]); IT.append(it[s:e]); CH.append(chg[s:e])
        PM.append(pmz[0] + rng.uniform(-300, 300) if r < 400 else pmz[r])
        offs.append(offs[-1] + (e - s))
    lib = PackedSpectra.from_numpy(np.asarray(offs, np.int32), np.concatenate(MZ), np.concatenate(IT),
                                   np.concatenate(CH), np.asarray(PM), pz)
    return lib0, aux, lib


def tie_queries(lib0, aux, nq, seed, with_copies=0):
    """queries of make_queries; the first `with_copies` become row 0's spectrum (the tie block's)."""
    from ann_solo_amd import synthetic
    from ann_solo_amd.packed import PackedSpectra
    q, _ = synthetic.make_queries(lib0, aux, nq, seed=seed, charge=2)
    qo, qmz, qit, qchg, qpmz, qpz = q.numpy()
    o, mz, it, chg, pmz, pz = lib0.numpy()
    a, b = int(o[0]), int(o[1])
    offs, MZ, IT, CH = [0], [], [], []
    for i in range(q.n):
        s, e = int(qo[i]), int(qo[i + 1])
        src = (mz[a:b], it[a:b], chg[a:b]) if i < with_copies else (qmz[s:e], qit[s:e], qchg[s:e])
        MZ.append(src[0]); IT.append(src[1]); CH.append(src[2])
        offs.append(offs[-1] + len(src[0]))
    qp = np.array(qpmz, np.float64)
    qp[:with_copies] = pmz[0] + 7.0
    return PackedSpectra.from_numpy(np.asarray(offs, np.int32), np.concatenate(MZ), np.concatenate(IT),
                                    np.concatenate(CH), qp, qpz)


def encode(O, spectra):
    o, mz, it, *_ = spectra.numpy()
    _, min_bound, _ = O.get_dim(11, 2010, 0.04)
    return O.encode_batch(mz, it, o, min_bound, 0.04, 800)
