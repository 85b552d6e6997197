"""The reference of an IVF-PQ index with FAISS' ``by_residual = false``, built from the oracle as it
stands (a helper, not a test). The oracle quantises residuals ``x - centroid[list]``: against a
one-row table of zeros the residual of every vector is the vector itself (``x - 0.0f`` is ``x``, bit
for bit), and neither the training subsample nor the seeds depend on the centroids, so ``pq_train`` /
``pq_encode`` give the raw-vector quantiser and codes. The score is FAISS' ``dis0 + sum_m
LUT[m][code_m]`` with ``dis0 = 0``: ``O.adc(lut, code, 0.0)``, restated here in float32 numpy over
whole lists (``adc_tree``; tests/test_pq_by_residual_cpu.py holds it bit-equal to the oracle's)."""
import numpy as np

PAD_D = np.float32(-3.4028234663852886e38)      # -FLT_MAX: what the oracle (and FAISS) pad D with; I gets -1


def raw_quantiser(O, xb, m, ksub, niter, seed):
    """(codebooks [m, ksub, d / m], codes [n, m]) of the raw vectors ``xb``."""
    xb = np.ascontiguousarray(xb, np.float32)
    zero = np.zeros((1, xb.shape[1]), np.float32)
    cb = O.pq_train(xb, zero, m, ksub, niter, seed)
    return cb, raw_codes(O, xb, cb)


def raw_codes(O, xb, cb):
    xb = np.ascontiguousarray(xb, np.float32)
    return O.pq_encode(xb, np.zeros((1, xb.shape[1]), np.float32), np.zeros(len(xb), np.int32), cb)


def adc_tree(lut, codes):
    """``O.adc(lut, code, 0.0)`` for every row of ``codes`` [n, m] (float32 [n]): 16 strided partials
    (sub-quantisers j, j + 16, ... added in that order; 0 where there is none), the mirror adds
    (j, 15 - j), (j, 7 - j), (j, 3 - j), then ``0.0f + (p0 + p1)``."""
    lut = np.ascontiguousarray(lut, np.float32)
    codes = np.asarray(codes)
    n, m = codes.shape
    v = lut[np.arange(m)[None, :], codes]                  # [n, m] float32
    p = np.zeros((n, 16), np.float32)
    for j in range(min(16, m)):
        a = v[:, j].copy()
        for mi in range(j + 16, m, 16):
            a = a + v[:, mi]
        p[:, j] = a
    for half in (8, 4, 2):
        for j in range(half):
            p[:, j] = p[:, j] + p[:, 2 * half - 1 - j]
    return np.float32(0.0) + (p[:, 0] + p[:, 1])


def _rank(scores, ids, k):
    """Top-k rows by (score descending, id ascending), padded with (-FLT_MAX, -1)."""
    order = np.lexsort((ids, -scores.astype(np.float64)))[:k]
    D = np.full(k, PAD_D, np.float32)
    I = np.full(k, -1, np.int64)
    D[:len(order)] = scores[order]
    I[:len(order)] = ids[order]
    return D, I


def raw_search(O, xq, cen, ivf, k, nprobe, keep=None):
    """(D [nq, k], I [nq, k]) of the raw-code index: probes by ``O.coarse`` (the centroids still define
    the lists), every vector of a probed list scored ``adc_tree`` of the query's ``O.pq_lut``. ``ivf``: an
    ``O.HostIVF`` over the raw codes and codebooks. ``keep`` (bool [nq, ntotal], optional): only the
    vectors a query's row keeps take part -- the window scan."""
    xq = np.ascontiguousarray(xq, np.float32)
    nprobe = min(nprobe, ivf.nlist)
    _, cI = O.coarse(xq, cen, nprobe)
    off = ivf.list_offsets
    D = np.empty((len(xq), k), np.float32)
    I = np.empty((len(xq), k), np.int64)
    for q in range(len(xq)):
        pos = np.concatenate([np.arange(off[l], off[l + 1]) for l in cI[q] if l >= 0] + [np.zeros(0, np.int64)])
        pos = pos.astype(np.int64)
        ids = ivf.ids[pos].astype(np.int64)
        if keep is not None:
            sel = keep[q][ids]
            pos, ids = pos[sel], ids[sel]
        sc = adc_tree(O.pq_lut(xq[q], ivf.codebooks), ivf.payload[pos])
        D[q], I[q] = _rank(sc, ids, k)
    return D, I
