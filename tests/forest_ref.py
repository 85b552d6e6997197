"""The histogram forest of ``asl_forest_bin`` / ``asl_forest_fit`` / ``asl_forest_predict`` (include/annsolo_mi.h,
csrc/forest.hip; DESIGN.md 3 "Rescoring model: forest") restated in numpy: the same hash, bootstrap, column draws,
binning, split rule in the same fp64 order, heap layout and truncated prediction. Every count is an integer and
every fp64 expression is written once, operation by operation, so the device reproduces these arrays bit for bit
(tests/test_gpu_forest.py). The functions have the signatures of ``ann_solo_amd._lib.forest_*``; ``SOLVER`` is the
triple ``fdr.ForestTDC(solver=...)`` takes.

The restatement works on the OCCUPIED bins of a (node, slot) histogram only. The device walks all 256: an empty
bin repeats the left-hand counts of the occupied bin before it, hence its proxy bit for bit, and the lowest bin of
equal proxies wins -- the occupied one."""
import numpy as np

MAX_BINS = 256
MAX_DEPTH = 12
NODES = (1 << (MAX_DEPTH + 1)) - 1
ROW = 64
_M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------ the draws
def mix(x):
    """The 32-bit finaliser of every draw, on uint64 arrays that hold 32-bit values."""
    x = np.asarray(x, np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & _M32
    return x ^ (x >> np.uint64(16))


def hash3(seed, a, b, c):
    """``fo_hash(seed, a, b, c)``: the finaliser after every key word."""
    h = mix(np.uint64(int(seed) & 0xFFFFFFFF) + np.uint64(0x9e3779b9))
    h = mix(h + np.asarray(a, np.uint64))
    h = mix(h + np.asarray(b, np.uint64))
    return mix(h + np.asarray(c, np.uint64))


def draw(h, m):
    """A hash to 0 .. m - 1 by multiply-and-shift."""
    return ((np.asarray(h, np.uint64) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def bootstrap(seed: int, trees: int, n: int) -> np.ndarray:
    """``mult [trees, n]``: tree t draws n rows with replacement from all n rows; draw j is keyed (seed, 2 t, j)."""
    mult = np.zeros((trees, n), np.int64)
    j = np.arange(n, dtype=np.uint64)
    for t in range(trees):
        if n:
            mult[t] = np.bincount(draw(hash3(seed, 2 * t, j, 0), n), minlength=n)
    return mult


def mtry_of(d: int) -> int:
    return max(1, int(np.floor(np.sqrt(d))))


def draw_columns(seed: int, t: int, d: int) -> np.ndarray:
    """``cols [NODES, mtry]``: per node of tree t in heap order, mtry distinct columns in draw order; draw k is keyed
    (seed, 2 t + 1, node, k) and picks the r-th column not drawn yet, r in 0 .. d - k - 1."""
    mtry = mtry_of(d)
    node = np.arange(NODES, dtype=np.uint64)
    cols = np.zeros((NODES, mtry), np.int64)
    for k in range(mtry):
        c = draw(hash3(seed, 2 * t + 1, node, k), d - k)
        taken = np.sort(cols[:, :k], axis=1)
        for j in range(k):
            c = c + (c >= taken[:, j])
        cols[:, k] = c
    return cols


# ------------------------------------------------------------------------------------------ binning
def bin_edges(X, train=None):
    """``(edges [d, 255], n_edges [d])``: per column the order statistics of its values over the rows ``train`` at
    the ranks ``floor(k * n_train / 256)``, k = 1 .. 255, duplicates removed -- no interpolation."""
    X = np.asarray(X, np.float64)
    Xt = X if train is None else X[train]
    nt, d = Xt.shape
    edges, n_edges = np.zeros((d, MAX_BINS - 1)), np.zeros(d, np.int32)
    if nt:
        ranks = (np.arange(1, MAX_BINS) * nt) // MAX_BINS
        S = np.sort(Xt, axis=0)[ranks]
        for j in range(d):
            e = np.unique(S[:, j])
            edges[j, :len(e)], n_edges[j] = e, len(e)
    return edges, n_edges


def forest_bin(X, edges, n_edges) -> np.ndarray:
    """``_lib.forest_bin``: byte j of row i = the number of edges of column j below ``X[i, j]`` (none is below a
    NaN)."""
    X = np.asarray(X, np.float64)
    n, d = X.shape
    out = np.zeros((n, ROW), np.uint8)
    for j in range(d):
        out[:, j] = (edges[j, :n_edges[j]][None, :] < X[:, j][:, None]).sum(axis=1)
    return out


# ------------------------------------------------------------------------------------------ the model
class Model:
    """The arrays of ``_lib.ForestModel``: ``[P, trees, NODES]``."""

    def __init__(self, P, trees, max_depth):
        self.P, self.trees, self.max_depth = P, trees, max_depth
        shape = (P, trees, NODES)
        self.col = np.full(shape, -1, np.int16)
        self.bin = np.zeros(shape, np.uint8)
        self.n0, self.n1 = np.zeros(shape, np.uint32), np.zeros(shape, np.uint32)
        self.value = np.zeros(shape)
        self.value[:, :, 0] = 0.5           # a problem without rows

    def numpy(self):
        return dict(col=self.col, bin=self.bin, n0=self.n0, n1=self.n1, value=self.value)


def node_value(cw0, cw1, n0, n1):
    """w1 / (w0 + w1), 0.5 where the node has no weight."""
    w0, w1 = cw0 * n0.astype(np.float64), cw1 * n1.astype(np.float64)
    w = w0 + w1
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(w > 0.0, w1 / w, 0.5)


def side(a0, a1):
    """(a1^2 + a0^2) / (a0 + a1): one side of the proxy and the parent's bound, in this order of operations."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return (a1 * a1 + a0 * a0) / (a0 + a1)


def forest_fit(bins, d, label, cw, trees=100, max_depth=MAX_DEPTH, seed=1, n_bins=None, mult=None) -> Model:
    """``_lib.forest_fit``. ``mult``: multiplicities to use in place of the bootstrap's (for the tests)."""
    bins = np.asarray(bins)
    label = np.asarray(label, np.int8)
    cw = np.asarray(cw, np.float64)
    n, (P, _) = bins.shape[0], label.shape
    if not 1 <= d <= ROW - 1 or not 1 <= max_depth <= MAX_DEPTH or trees < 1 or bins.shape[1] != ROW:
        raise ValueError('forest_fit: shape or limits')
    if np.any((label < -1) | (label > 1)) or not np.all(np.isfinite(cw) & (cw >= 0)):
        raise ValueError('forest_fit: labels in {-1, 0, +1}, finite class weights >= 0')
    if n_bins is not None and n and np.any(bins[:, :d] >= np.asarray(n_bins)[None, :]):
        raise ValueError('forest_fit: a bin beyond its column')
    mtry = mtry_of(d)
    M = Model(P, trees, max_depth)
    if n == 0:
        return M
    mult = bootstrap(seed, trees, n) if mult is None else np.asarray(mult, np.int64)
    for t in range(trees):
        cols = draw_columns(seed, t, d)
        pp, rows = np.nonzero((label != 0) & (mult[t] > 0)[None, :])       # in the problem and in the bag
        m = mult[t][rows]
        cls = (label[pp, rows] > 0).astype(np.int64)
        node = np.zeros(len(pp), np.int64)
        col, sbin, n0, n1, value = M.col[:, t], M.bin[:, t], M.n0[:, t], M.n1[:, t], M.value[:, t]
        root = np.bincount(pp * 2 + cls, weights=m, minlength=2 * P).astype(np.int64).reshape(P, 2)
        has = root.sum(axis=1) > 0
        n0[has, 0], n1[has, 0] = root[has, 0], root[has, 1]
        value[has, 0] = node_value(cw[has, 0], cw[has, 1], root[has, 0], root[has, 1])
        for level in range(max_depth):
            if len(pp) == 0:
                break
            if level:       # partition: every row to the child its node's split names; a leaf keeps none
                c = col[pp, node].astype(np.int64)
                go = c >= 0
                pp, rows, m, cls, node, c = pp[go], rows[go], m[go], cls[go], node[go], c[go]
                node = 2 * node + 1 + (bins[rows, c] > sbin[pp, node])
                if len(pp) == 0:
                    break
            # histogram: the occupied (problem, node, slot, bin) entries with their class counts
            k = np.repeat(np.arange(mtry), len(pp))
            rr, pn = np.tile(rows, mtry), np.tile(pp * NODES + node, mtry)
            key = (pn * mtry + k) * MAX_BINS + bins[rr, cols[np.tile(node, mtry), k]]
            uk, inv = np.unique(key, return_inverse=True)
            h1 = np.bincount(inv, weights=np.tile(m * cls, mtry), minlength=len(uk)).astype(np.int64)
            h0 = np.bincount(inv, weights=np.tile(m * (1 - cls), mtry), minlength=len(uk)).astype(np.int64)
            # left-hand counts: running sums inside each (problem, node, slot)
            seg = uk // MAX_BINS
            start = np.nonzero(np.append(True, seg[1:] != seg[:-1]))[0]
            seg_id = np.cumsum(np.append(True, seg[1:] != seg[:-1])) - 1
            c0, c1 = np.cumsum(h0), np.cumsum(h1)
            l0 = c0 - (c0[start] - h0[start])[seg_id]
            l1 = c1 - (c1[start] - h1[start])[seg_id]
            e_pn = seg // mtry
            e_p, e_node = e_pn // NODES, e_pn % NODES
            N0, N1 = n0[e_p, e_node].astype(np.int64), n1[e_p, e_node].astype(np.int64)
            r0, r1 = N0 - l0, N1 - l1
            cw0, cw1 = cw[e_p, 0], cw[e_p, 1]
            wl0, wl1, wr0, wr1 = cw0 * l0, cw1 * l1, cw0 * r0, cw1 * r1
            ok = (N0 != 0) & (N1 != 0) & (l0 + l1 >= 1) & (r0 + r1 >= 1) & (wl0 + wl1 > 0.0) & (wr0 + wr1 > 0.0)
            with np.errstate(invalid='ignore'):
                proxy = np.where(ok, side(wl0, wl1) + side(wr0, wr1), -np.inf)
            # per (problem, node): the highest proxy; of equals the first slot, then the lowest bin (= key order)
            g_start = np.nonzero(np.append(True, e_pn[1:] != e_pn[:-1]))[0]
            g_id = np.cumsum(np.append(True, e_pn[1:] != e_pn[:-1])) - 1
            g_max = np.maximum.reduceat(proxy, g_start)
            idx = np.arange(len(uk))
            first = np.minimum.reduceat(np.where(proxy == g_max[g_id], idx, len(uk)), g_start)
            g_p, g_node = e_p[g_start], e_node[g_start]
            G0, G1 = n0[g_p, g_node].astype(np.float64), n1[g_p, g_node].astype(np.float64)
            parent = side(cw[g_p, 0] * G0, cw[g_p, 1] * G1)
            split = g_max > parent                      # strictly; -inf (no candidate) and NaN never do
            f, sp, sn = first[split], g_p[split], g_node[split]
            col[sp, sn] = cols[sn, (uk[f] // MAX_BINS) % mtry]
            sbin[sp, sn] = uk[f] % MAX_BINS
            for child, a0, a1 in ((2 * sn + 1, l0[f], l1[f]), (2 * sn + 2, r0[f], r1[f])):
                n0[sp, child], n1[sp, child] = a0, a1
                value[sp, child] = node_value(cw[sp, 0], cw[sp, 1], a0, a1)
    return M


def forest_predict(bins, d, model, max_depth=None) -> np.ndarray:
    """``_lib.forest_predict``: ``proba [P, n]``, the values summed in tree order, then divided by the tree count."""
    bins = np.asarray(bins)
    n, P = bins.shape[0], model.P
    depth = model.max_depth if max_depth is None else int(max_depth)
    if not 0 <= depth <= MAX_DEPTH:
        raise ValueError('forest_predict: max_depth')
    acc = np.zeros((P, n))
    pi, ri = np.arange(P)[:, None], np.arange(n)[None, :]
    for t in range(model.trees):
        col, sbin, value = model.col[:, t], model.bin[:, t], model.value[:, t]
        node = np.zeros((P, n), np.int64)
        for _ in range(depth):
            c = col[pi, node].astype(np.int64)
            go = c >= 0
            if not go.any():
                break
            right = bins[ri, np.maximum(c, 0)] > sbin[pi, node]
            node = np.where(go, 2 * node + 1 + right, node)
        acc = acc + value[pi, node]
    return acc / float(model.trees)


SOLVER = (forest_bin, forest_fit, forest_predict)
