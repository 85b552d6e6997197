"""The shifted dot product with a PER-PEAK fragment tolerance, restated in numpy / Python: the
yardstick of the ppm fragment mode (include/annsolo_mi.h: ASL_SCORE_FRAGMENT_PPM).

It follows SpectrumMatcher::dot the way the CPU oracle does (oracle/asl_oracle.c: orc_dot_pair) with
one change: wherever the sweep reads the tolerance for query peak i it reads ``tol_i``.

    unit 'Da' :  tol_i = tol for every peak, the shift gate reads tol          (the oracle, bit for bit:
                 tests/test_ppm_cpu.py holds the two against each other)
    unit 'ppm':  rel = tol * 1e-6 (one fp64 multiply), tol_i = rel * (double)q_mz[i] (one fp64 multiply),
                 the shift gate reads rel * q_pmz

Every number below is an fp64 numpy scalar or array, every operation one IEEE operation (numpy does
not contract a multiply and an add), products are rounded to float32 as the reference's tuple store
does. Spectra come as the six packed arrays of tests/rescore_cases.py:
(offsets, mz, intensity, charge, precursor_mz, precursor_charge)."""
import numpy as np


def rel_tol(tol):
    return np.float64(tol) * np.float64(1e-6)


def peak_tol(q_mz, tol, unit):
    """tol_i of every query peak (float64)."""
    q = np.asarray(q_mz, np.float32).astype(np.float64)
    if unit == 'Da':
        return np.full(len(q), np.float64(tol))
    assert unit == 'ppm', unit
    return rel_tol(tol) * q


def shift_gate(q_pmz, tol, unit):
    """The threshold |pmd| is held against (SpectrumMatch.cpp:20)."""
    return np.float64(tol) if unit == 'Da' else rel_tol(tol) * np.float64(q_pmz)


def num_shifts(q_pmz, c_pmz, c_charge, tol, allow_shift, unit):
    pmd = (np.float64(q_pmz) - np.float64(c_pmz)) * np.float64(int(c_charge) & 0xffffffff)
    n = int(c_charge) + 1 if (allow_shift and abs(pmd) >= shift_gate(q_pmz, tol, unit)) else 1
    return min(n, 64), pmd                    # (the oracle's shift table holds 64)


def generated(q_mz, q_pmz, c_mz, c_chg, c_pmz, c_charge, tol, allow_shift, unit):
    """The peak matches the sweep generates, in generation order (query peak, shift, candidate peak):
    int arrays (qi, s, ci) and the factor (1 or 2/3) of each."""
    qn, cn = len(q_mz), len(c_mz)
    if qn <= 0 or cn <= 0:
        z = np.zeros(0, np.int64)
        return z, z, z, np.zeros(0)
    qm = np.asarray(q_mz, np.float32).astype(np.float64)
    cm = np.asarray(c_mz, np.float32).astype(np.float64)
    chg = np.asarray(c_chg).astype(np.int64)
    tl = peak_tol(q_mz, tol, unit)
    S, pmd = num_shifts(q_pmz, c_pmz, c_charge, tol, allow_shift, unit)
    lim = qm - tl
    out = []
    for s in range(S):
        md = np.float64(0.0) if s == 0 else pmd / np.float64(s)
        x = cm + md                                            # ascends with the candidate's peaks
        # the running cursor: advanced while cursor < cn - 1 and lim_i > x[cursor]. x ascends, so the
        # sweep for peak i alone stops at min(#(x < lim_i), cn - 1), and starting from the cursor of
        # peak i - 1 it stops at the larger of the two
        below = lim[:, None] > x[None, :]
        assert np.all(below[:, :-1] >= below[:, 1:]), 'candidate peaks ascend'
        first = np.minimum(below.sum(axis=1), cn - 1)
        cursor = np.maximum.accumulate(first)
        ok = np.abs(qm[:, None] - x[None, :]) <= tl[:, None]   # the window test, every (i, j)
        j = np.arange(cn)[None, :]
        # from the cursor on, up to the first peak outside the window
        stop = np.where((j >= cursor[:, None]) & ~ok, j, cn).min(axis=1)
        take = (j >= cursor[:, None]) & (j < stop[:, None])
        if s > 0:
            take &= ((chg == s) | (chg == 0))[None, :]
        qi, ci = np.nonzero(take)
        mult = np.where((s == 0) | (chg[ci] == s), 1.0, 2.0 / 3.0)
        out.append((qi, np.full(len(qi), s, np.int64), ci, mult))
    qi, sh, ci, mult = (np.concatenate([o[k] for o in out]) for k in range(4))
    order = np.lexsort((ci, sh, qi))
    return qi[order], sh[order], ci[order], mult[order]


def dot_pair(q_mz, q_int, q_pmz, c_mz, c_int, c_chg, c_pmz, c_charge, tol, allow_shift, unit='ppm'):
    """(score, matches [n, 2] (query peak, candidate peak) in greedy order)."""
    qi, _, ci, mult = generated(q_mz, q_pmz, c_mz, c_chg, c_pmz, c_charge, tol, allow_shift, unit)
    if len(qi) == 0:
        return 0.0, np.zeros((0, 2), np.uint32)
    qv = np.asarray(q_int, np.float32).astype(np.float64)[qi]
    cv = np.asarray(c_int, np.float32).astype(np.float64)[ci]
    with np.errstate(over='ignore', under='ignore'):
        prod = ((mult * qv) * cv).astype(np.float32)              # cpp:81
    # product descending, ties in generation order (the oracle's insertion sort moves an entry only
    # past strictly smaller ones). NaN products do not occur in the cases.
    order = np.argsort(-prod.astype(np.float64), kind='stable')
    q_used, c_used = set(), set()
    score, matches = 0.0, []
    for t in order.tolist():
        a, b = int(qi[t]), int(ci[t])
        if a in q_used or b in c_used:
            continue
        score += float(prod[t])
        matches.append((a, b))
        q_used.add(a)
        c_used.add(b)
    return score, np.asarray(matches, np.uint32).reshape(-1, 2)


def spectrum(packed, r):
    o = packed[0]
    a = slice(int(o[r]), int(o[r + 1]))
    return packed[1][a], packed[2][a], packed[3][a], float(packed[4][r]), int(packed[5][r])


def pair(queries, q, library, r, tol, allow_shift=True, unit='ppm'):
    qmz, qit, _, qp, _ = spectrum(queries, q)
    cmz, cit, cch, cp, cz = spectrum(library, r)
    return dot_pair(qmz, qit, qp, cmz, cit, cch, cp, cz, tol, allow_shift, unit)


def scores(queries, q, library, rows, tol, allow_shift=True, unit='ppm'):
    return np.array([pair(queries, q, library, int(r), tol, allow_shift, unit)[0] for r in rows], np.float64)


def best_match(queries, q, library, rows, tol, allow_shift=True, unit='ppm'):
    """(position in `rows` of the first strict maximum, its score, its matches): get_best_match."""
    sc = scores(queries, q, library, rows, tol, allow_shift, unit)
    b = int(np.argmax(sc))                      # the first of equal maxima
    return b, float(sc[b]), pair(queries, q, library, int(rows[b]), tol, allow_shift, unit)[1]


def ranked(sc, n, keys=None):
    """Positions of the n best scores: score descending, then `keys` (default: position) ascending."""
    sc = np.asarray(sc, np.float64)
    keys = np.arange(len(sc)) if keys is None else np.asarray(keys)
    return np.lexsort((keys, -sc))[:n]
