"""``asl_ssm_groups`` restated in numpy from the comment of its declaration in include/annsolo_mi.h, without scipy:
``ssm_groups(md, min_group_size) -> (group int32 [n], n_peaks, n_labels, peak_mass float64 [n_peaks], peak_size
int64 [n_peaks])``. tests/test_groups_cpu.py holds it to ``fdr.ssm_groups`` byte for byte; the GPU test takes the
profile columns from it."""
import numpy as np

BINS = 100
MAX_SPAN = 65536


def edges(g: float) -> np.ndarray:
    """The 101 edges of the interval of nominal value ``g``: a rounded product, then a rounded sum (two ufunc
    calls: numpy does not fuse them); the last edge is g + 0.5."""
    e = np.arange(BINS, dtype=np.float64) * 0.01
    e = e + (g - 0.5)
    return np.append(e, g + 0.5)


def edges_contracted(g: float) -> np.ndarray:
    """What ``edges`` would be if product and sum were ONE rounding (an FMA): for the cases' own check."""
    from fractions import Fraction
    e = [float(Fraction(0.01) * i + Fraction(g - 0.5)) for i in range(BINS)]
    return np.array(e + [g + 0.5])


def bin_of(x: np.ndarray, e: np.ndarray) -> np.ndarray:
    """edge[i] <= x < edge[i + 1]; bin 99 also takes x == edge[100]."""
    i = np.searchsorted(e, x, side='right') - 1
    return np.clip(i, 0, BINS - 1)


def peaks_of(c) -> list:
    """Strict local maxima of the counts; a plateau once at (first + last) // 2; never bin 0 or 99, never a plateau
    that reaches bin 99."""
    out, i = [], 1
    while i < BINS - 1:
        if c[i - 1] < c[i]:
            j = i + 1
            while j < BINS - 1 and c[j] == c[i]:
                j += 1
            if c[j] < c[i]:
                out.append((i + j - 1) // 2)
                i = j
        i += 1
    return out


def bases_of(c, p: int):
    """Walk outward while the count is <= the peak's; the base is the minimum met, the nearest of equal minima."""
    left = right = p
    low = c[p]
    i = p
    while i >= 0 and c[i] <= c[p]:
        if c[i] < low:
            low, left = c[i], i
        i -= 1
    low = c[p]
    i = p
    while i < BINS and c[i] <= c[p]:
        if c[i] < low:
            low, right = c[i], i
        i += 1
    return left, right


def ssm_groups(md, min_group_size: int):
    md = np.asarray(md, np.float64)
    n = len(md)
    if min_group_size < 0:
        raise ValueError('min_group_size < 0')
    if not np.isfinite(md).all():
        raise ValueError('a non-finite mass difference')
    group = np.full(n, -1, np.int32)
    if n == 0:
        return group, 0, 0, np.zeros(0), np.zeros(0, np.int64)
    nominal = np.rint(md)
    if nominal.max() - nominal.min() + 1 > MAX_SPAN:
        raise OverflowError('span')
    mass, next_id = [], 0
    for g in np.unique(nominal):
        rows = np.nonzero(nominal == g)[0]
        if g == nominal.max() and len(rows) == 1:     # the last interval with one SSM is skipped (n == 1 too)
            continue
        e, x = edges(g), md[rows]
        c = np.bincount(bin_of(x, e), minlength=BINS)
        pk = peaks_of(c)
        best, arg = np.full(len(x), np.inf), np.full(len(x), -1)
        for k, p in enumerate(pk):
            lb, rb = bases_of(c, p)
            dist = np.where((e[lb] < x) & (x < e[rb]), np.abs(e[p] - x), np.inf)
            better = dist < best                    # strict: equal distances stay with the lower index
            best[better], arg[better] = dist[better], k
        group[rows[arg >= 0]] = (next_id + arg[arg >= 0]).astype(np.int32)
        mass += [e[p] for p in pk]
        next_id += len(pk)
    size = np.bincount(group[group >= 0], minlength=next_id).astype(np.int64)
    small = np.nonzero(size < min_group_size)[0]
    group[np.isin(group, small)] = -1
    return group, next_id, len(np.unique(group)), np.array(mass, np.float64).reshape(-1), size
