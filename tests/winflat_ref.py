"""Reference of the window-exact index (`ASL_INDEX_WINFLAT`, `Config.index = 'winflat'`): numpy and the oracle
only, nothing from the package's device path. For a query, `keep = precursor_ok` over the key column; its
neighbours are the oracle's exact flat search over the kept vectors, ids mapped back; the fused path is the
oracle's batch over a one-list `HostIVF` (built by hand, nprobe 1) that holds only the kept vectors."""
import numpy as np

from test_gpu_window_scan import _window_mask

NEG = np.float32(-3.402823466e+38)


def interval_mask(lo, hi, key):
    """lo <= (double)key <= hi; a NaN key or bound never passes, lo > hi is empty, +-inf are legal bounds."""
    l = np.asarray(key, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore'):
        return (lo <= l) & (l <= hi)


def mask(q, key, charge, tol, mode):
    """`q`: the query's precursor m/z ('Da', 'ppm') or its (lo, hi) pair ('interval')."""
    if mode == 'interval':
        return interval_mask(float(q[0]), float(q[1]), key)
    return _window_mask(float(q), key, charge, tol, mode)


def search(O, xb, xq, k, keeps):
    """(D, I) [nq, k]: the k best (score desc, id asc) of xb[keeps[i]] for query i, -1 / -FLT_MAX padded."""
    nq = len(xq)
    D = np.full((nq, k), NEG, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        ids = np.flatnonzero(keeps[i])
        if len(ids) == 0:
            continue
        d, j = O.flat_search(xb[ids], xq[i:i + 1], k)
        v = j[0] >= 0
        I[i, v] = ids[j[0][v]]
        D[i, v] = d[0][v]
    return D, I


def one_list_ivf(O, xb, keep):
    """The oracle's IVF with ONE list that holds the kept vectors, ascending id (searched with nprobe 1)."""
    ids = np.flatnonzero(keep).astype(np.int32)
    ivf = O.HostIVF.__new__(O.HostIVF)
    ivf.d = xb.shape[1]
    ivf.centroids, ivf.nlist, ivf.codebooks, ivf.kind = np.zeros((1, ivf.d), np.float32), 1, None, 0
    ivf.list_offsets = np.array([0, len(ids)], np.int32)
    ivf.ids = ids
    ivf.payload = np.ascontiguousarray(xb[ids], np.float32).reshape(len(ids), ivf.d)
    return ivf


def spectra_rows(O, q, rows):
    o, mz, it, chg, pmz, pz = q.numpy()
    sel = [(int(o[i]), int(o[i + 1])) for i in rows]
    offs = np.concatenate([[0], np.cumsum([e - s for s, e in sel])]).astype(np.int32)
    cat = lambda a: np.concatenate([a[s:e] for s, e in sel])
    return O.Spectra(offs, cat(mz), cat(it), cat(chg), pmz[list(rows)], pz[list(rows)])


def fused(O, q, i, L, xb, key, charge, keep, k, pm_stride, frag_tol=0.02):
    """The oracle's batch for query i over the kept vectors alone: the list holds nothing else, so the window
    the oracle applies behind its top-k is given a tolerance that every kept row passes."""
    return O.search_batch(spectra_rows(O, q, [i]), L, key, charge, one_list_ivf(O, xb, keep), k, 1, 1e12, 'Da',
                          frag_tol, True, pm_stride=pm_stride, want_knn=True)
