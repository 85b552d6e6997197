"""numpy restatement of ``asl_tdc_qvalues`` written from the comment of include/annsolo_mi.h and DESIGN.md 3
"Target-decoy q-values" -- the order key, one sort, integer prefix counts, one division per run end, a reverse
minimum per group -- NOT from ann_solo_amd/fdr.py: test_tdc_cpu.py shows that the two agree byte for byte."""
import numpy as np


def score_key(score, desc: bool) -> np.ndarray:
    """The order-preserving map of float64 to uint64 (ascending key = ascending score; -0.0 is +0.0), its
    complement for ``desc``."""
    s = np.array(score, np.float64)
    s[s == 0.0] = 0.0
    u = s.view(np.uint64)
    neg = (u >> np.uint64(63)) != 0
    key = np.where(neg, ~u, u | np.uint64(1 << 63))
    return ~key if desc else key


def group_key(group) -> np.ndarray:
    """int32 ids with the sign bit flipped: ascending as uint32 = ascending as int32."""
    return np.asarray(group, np.int32).view(np.uint32) ^ np.uint32(0x80000000)


def tdc_qvalues(score, is_target, group=None, use=None, desc=True, fdr=None):
    """``q [n]`` (NaN for unused rows) or, with ``fdr``, ``(q, label)``; ``ValueError`` where the entry point
    returns ASL_ERR_INVALID."""
    score = np.asarray(score, np.float64)
    n = len(score)
    target = np.asarray(is_target).astype(bool)
    used = np.ones(n, bool) if use is None else np.asarray(use) != 0
    if desc not in (0, 1, False, True):
        raise ValueError('desc')
    if fdr is not None and not fdr >= 0.0:
        raise ValueError('fdr')
    if np.isnan(score[used]).any():
        raise ValueError('a NaN score in a used row')
    q = np.full(n, np.nan)
    label = np.zeros(n, np.int8)
    rows = np.nonzero(used)[0]
    m = len(rows)
    if m:
        sk = score_key(score[rows], bool(desc))
        gk = np.zeros(m, np.uint32) if group is None else group_key(np.asarray(group)[rows])
        order = np.lexsort((sk, gk))                    # group major, score key minor
        sk, gk, idx, t = sk[order], gk[order], rows[order], target[rows][order]
        pos = np.arange(m, dtype=np.int64)
        head = np.maximum.accumulate(np.where(np.append(True, gk[1:] != gk[:-1]), pos, 0))
        cum_t = np.cumsum(t.astype(np.int64))
        t_before = cum_t[head] - t[head]
        nt = cum_t - t_before
        nd = (pos - head + 1) - nt
        end = np.append((gk[1:] != gk[:-1]) | (sk[1:] != sk[:-1]), True)
        v = np.full(m, np.inf)
        e = np.nonzero(end)[0]
        has = nt[e] != 0
        val = np.ones(len(e))
        val[has] = np.minimum((nd[e][has] + 1).astype(np.float64) / nt[e][has].astype(np.float64), 1.0)
        v[e] = val
        qs = np.empty(m)
        starts = np.nonzero(np.append(True, gk[1:] != gk[:-1]))[0]
        for a, b in zip(starts, np.append(starts[1:], m)):      # reverse minimum inside every group
            qs[a:b] = np.minimum.accumulate(v[a:b][::-1])[::-1]
        q[idx] = qs
        label[idx] = np.where(t, (qs <= (0.0 if fdr is None else fdr)).astype(np.int8), -1)
    return q if fdr is None else (q, label)
