"""The reference of a subset search (a helper, not a test): the oracle's IVF search over an index that
holds, in the same lists with the same centroids, codebooks and payload, only the selected vectors --
``_filtered`` of tests/test_gpu_window_scan.py for any payload -- and the key column of a library with a
selection (NaN where a row is unselected). numpy and the oracle only."""
import numpy as np


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
    """The IVF with only the vectors whose id is kept: same lists, same order inside a list."""
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


def search_selected(O, ivf, xq, k, nprobe, keep_by_id):
    """(D, I) [nq, k]: the k best selected vectors of the probed lists, (score desc, id asc), -1 padded."""
    return filtered(O, ivf, keep_by_id).search(xq, k, nprobe)


def search_all_then_select(O, ivf, xq, k, nprobe, keep_by_id):
    """The same rows another way: EVERY vector of the probed lists in the oracle's order (a search with
    k = the number of vectors), the unselected ones struck out, the first k kept."""
    keep_by_id = np.asarray(keep_by_id, bool)
    n = len(ivf.ids)
    Da, Ia = ivf.search(xq, max(n, 1), nprobe)
    D = np.full((len(xq), k), Da[0, -1] if n and (Ia[:, -1] < 0).all() else np.float32(-3.4028234663852886e38),
                np.float32)
    I = np.full((len(xq), k), -1, np.int64)
    for i in range(len(xq)):
        ok = Ia[i] >= 0
        ok[ok] = keep_by_id[Ia[i][ok]]
        m = min(k, int(ok.sum()))
        I[i, :m] = Ia[i][ok][:m]
        D[i, :m] = Da[i][ok][:m]
    return D, I


def post_filtered(I_plain, keep_by_id):
    """Per row: the ids of a PLAIN search that are selected -- what a filter behind the top-k leaves."""
    keep_by_id = np.asarray(keep_by_id, bool)
    return [row[row >= 0][keep_by_id[row[row >= 0]]] for row in np.asarray(I_plain)]


def key_with_selection(key, keep_by_id):
    """The float32 key column of a library with a selection: NaN where the row is unselected."""
    out = np.array(key, np.float32)
    out[~np.asarray(keep_by_id, bool)] = np.nan
    return out


def assert_rows_equal(got, want, what=''):
    """ids equal and, where a row holds a hit, score bits equal."""
    (D, I), (rD, rI) = got, want
    assert np.array_equal(I, rI), what
    v = rI >= 0
    assert np.array_equal(np.asarray(D)[v].view(np.uint32), np.asarray(rD)[v].view(np.uint32)), what
