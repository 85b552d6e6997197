"""Rescoring cases for the pruning of deferred candidates (csrc/rescore.hip).

``rescore_flat_kernel`` cannot score a candidate in which a peak is matched twice (it is "deferred"
to the pair kernel), but it holds the sum of ALL generated matches of the pair: an upper bound of the
score, which sums a subset of the same non-negative products. In a winner-only request a deferred
candidate whose bound lies below the best exact score of the query is dropped ("pruned").

Plain numpy, no GPU, in the style of tests/rescore_cases.py. A case is a set of queries (1, 37 and
100 peaks on a 10 Da grid, tolerance 0.02) with a list of candidates each, planted so that it is
known which candidates are deferred and which of those are pruned: the margins are wide (bound
<= 0.5 x best for the prunable ones, bound >= best + 1e-3 for the others), so the kernels' counters
are exactly predictable. ``match_list`` is a port of the generation loop of ``orc_dot_pair``
(oracle/asl_oracle.c), which the kernels' accumulated sum follows match for match;
tests/test_rescore_prune_cpu.py checks it and the planted margins against the oracle,
tests/test_gpu_rescore_prune.py runs the cases through the kernels."""
from dataclasses import dataclass, field

import numpy as np

import rescore_cases as RC

TOL = 0.02
QN = (1, 37, 100)
N_CAND = 40                 # a full 32-candidate wave chunk and a second one
PMZ = 650.0                 # the queries' precursor m/z (charge 2)
PRUNE_REL, PRUNE_ABS = 1e-9, 1e-12      # the kernels' slack (RS_PRUNE_REL / RS_PRUNE_ABS)


# ------------------------------------------------------------------ the reference's match list
def match_list(q_mz, q_int, q_pmz, c_mz, c_int, c_chg, c_pmz, c_charge, tol, allow_shift):
    """The generated matches of a pair, [(product fp32, query peak, candidate peak)] in generation
    order: orc_dot_pair's loop, running cursors included (SpectrumMatch.cpp:18-87)."""
    q_n, c_n = len(q_mz), len(c_mz)
    if q_n <= 0 or c_n <= 0:
        return []
    pmd = (float(q_pmz) - float(c_pmz)) * float(np.uint32(c_charge))
    ns = min(int(c_charge) + 1 if (allow_shift and abs(pmd) >= tol) else 1, 64)
    cursor = [0] * ns
    md = [0.0] + [pmd / float(s) for s in range(1, ns)]
    cm = [float(x) for x in np.asarray(c_mz, np.float32)]
    out = []
    for qi in range(q_n):
        qm = float(np.float32(q_mz[qi]))
        for s in range(ns):
            while cursor[s] < c_n - 1 and qm - tol > cm[cursor[s]] + md[s]:
                cursor[s] += 1
        for s in range(ns):
            ci = cursor[s]
            while ci < c_n and abs(qm - (cm[ci] + md[s])) <= tol:
                mult = 1.0 if (s == 0 or c_chg[ci] == s) else (2.0 / 3.0 if c_chg[ci] == 0 else 0.0)
                if mult > 0.0:
                    out.append((np.float32(mult * float(np.float32(q_int[qi])) * float(np.float32(c_int[ci]))),
                                qi, ci))
                ci += 1
    return out


def bound_of(matches):
    """The sum of all generated products (fp64, generation order) and whether the kernels defer the
    pair: a query or candidate peak occurs twice, or a product is negative or NaN."""
    total = 0.0
    for p, _, _ in matches:
        total += float(p)
    qs = [q for _, q, _ in matches]
    cs = [c for _, _, c in matches]
    repeats = len(set(qs)) < len(qs) or len(set(cs)) < len(cs)
    signed = any(not (float(p) >= 0.0) for p, _, _ in matches)
    return total, repeats, signed


# ------------------------------------------------------------------ planting
def _grid(qn):
    return (200.0 + 10.0 * np.arange(qn)).astype(np.float32)


def _query(rng, qn):
    return _grid(qn), rng.uniform(0.3, 0.6, qn).astype(np.float32), np.zeros(qn, np.uint8)


def _cand(qmz, qint, parts):
    """A candidate from (query peak, m/z offset, product): its peak sits at qmz[i] + offset with the
    intensity that gives about that product (the exact value is whatever fp32 makes of it)."""
    mz = np.array([np.float32(np.float64(qmz[i]) + off) for i, off, _ in parts], np.float32)
    it = np.array([p / float(qint[i]) for i, _, p in parts], np.float32)
    order = np.argsort(mz, kind='stable')
    assert np.all(np.diff(mz[order]) > 0)
    return mz[order], it[order], np.zeros(len(parts), np.uint8)


def _split(rng, total, n):
    w = rng.uniform(0.5, 1.5, n)
    return total * w / w.sum()


def plain(rng, qmz, qint, total, npk=5, avoid=()):
    """Matches npk distinct query peaks once each: scored by the flat kernel, score ~ total."""
    pool = np.array([i for i in range(len(qmz)) if i not in avoid])
    picks = rng.choice(pool, min(npk, len(pool)), replace=False)
    return _cand(qmz, qint, [(int(i), float(rng.uniform(-0.01, 0.01)), float(p))
                             for i, p in zip(picks, _split(rng, total, len(picks)))])


def twin(rng, qmz, qint, exact, extra, npk=5, avoid=(), first=None):
    """plain(total = exact) plus a second peak in the window of its first query peak, with the
    smaller product `extra` (below the product already there, `first` if given): deferred, score ~
    exact, bound ~ exact + extra."""
    pool = np.array([i for i in range(len(qmz)) if i not in avoid])
    picks = rng.choice(pool, min(npk, len(pool)), replace=False)
    if first is None or len(picks) == 1:
        prods = _split(rng, exact, len(picks))
    else:
        prods = np.concatenate([[first], _split(rng, exact - first, len(picks) - 1)])
    assert extra < prods[0], (extra, prods[0])
    parts = [(int(picks[0]), -0.006, float(prods[0])), (int(picks[0]), 0.006, float(extra))]
    parts += [(int(i), float(rng.uniform(-0.01, 0.01)), float(p)) for i, p in zip(picks[1:], prods[1:])]
    return _cand(qmz, qint, parts)


@dataclass
class Case:
    name: str
    queries: tuple                 # packed arrays (offsets, mz, intensity, charge, precursor m/z, charge)
    library: tuple
    lists: list                    # per query: library rows in the caller's order (int64)
    notes: dict = field(default_factory=dict)

    def packed(self):
        from ann_solo_amd.packed import PackedSpectra
        return PackedSpectra.from_numpy(*self.queries), PackedSpectra.from_numpy(*self.library)

    @property
    def nq(self):
        return len(self.lists)

    def csr(self):
        off = np.concatenate([[0], np.cumsum([len(c) for c in self.lists])]).astype(np.int32)
        return np.concatenate(self.lists).astype(np.int64), off


def _assemble(name, per_query, notes=None, order='reversed'):
    """per_query: [(query spectrum, [candidate spectra], candidate precursor m/z or None)]. A query's
    rows are consecutive; its list names them in DESCENDING row order (so that position order and
    row order disagree: ties go different ways under the two rules)."""
    qs, lib, lists, l_pmz = [], [], [], []
    for q, cands, pmz in per_query:
        base = len(lib)
        lib += cands
        l_pmz += [PMZ] * len(cands) if pmz is None else list(pmz)
        rows = np.arange(base, base + len(cands), dtype=np.int64)
        lists.append(rows[::-1].copy() if order == 'reversed' else rows)
        qs.append(q)
    return Case(name, RC.pack(qs, [PMZ] * len(qs), [2] * len(qs)), RC.pack(lib, l_pmz, [2] * len(lib)),
                lists, notes or {})


def _fill(rng, qmz, qint, cands, n, lo, hi, low_bound, avoid=()):
    """Up to n candidates: plain ones scoring in [lo, hi] and, every fifth, a twin whose BOUND is
    at most low_bound (prunable). Every second candidate has a precursor 1.5 m/z below the query's
    (pmd = 3: three shifts, which match nothing on the 10 Da grid)."""
    k = 0
    while len(cands) < n:
        if k % 5 == 4:
            b = float(rng.uniform(0.5, 1.0)) * low_bound
            cands.append(twin(rng, qmz, qint, 0.8 * b, 0.2 * b / max(min(5, len(qmz)), 1) * 0.5, avoid=avoid))
        else:
            cands.append(plain(rng, qmz, qint, float(rng.uniform(lo, hi)), avoid=avoid))
        k += 1
    return cands


def _pmz_alternating(n):
    return [PMZ if i % 2 == 0 else PMZ - 1.5 for i in range(n)]


def case_a(seed=1):
    """The winner is itself deferred (a twin) and has the highest bound: not pruned, wins."""
    rng = np.random.default_rng(seed)
    per = []
    for qn in QN:
        q = _query(rng, qn)
        cands = [plain(rng, q[0], q[1], 0.30)]                          # best exact score
        cands.append(twin(rng, q[0], q[1], 0.90, 0.02))                 # exact 0.9, bound 0.92
        _fill(rng, q[0], q[1], cands, N_CAND, 0.05, 0.25, 0.15)
        per.append((q, cands, _pmz_alternating(N_CAND)))
    return _assemble('a', per, {'winner_local': 1})


def case_b(seed=2):
    """A deferred candidate with bound above and exact score below the best exact score (a twin with
    a large product): goes to the pair kernel and loses."""
    rng = np.random.default_rng(seed)
    per = []
    for qn in QN:
        q = _query(rng, qn)
        cands = [plain(rng, q[0], q[1], 0.40)]                          # the winner
        cands.append(twin(rng, q[0], q[1], 0.35, 0.10, first=0.15))    # exact ~0.35 < 0.40 < bound ~0.45
        _fill(rng, q[0], q[1], cands, N_CAND, 0.05, 0.30, 0.20)
        per.append((q, cands, _pmz_alternating(N_CAND)))
    return _assemble('b', per, {'winner_local': 0, 'loser_local': 1})


def case_c(seed=3):
    """A tie: Y is X plus one extra peak that doubly matches a query peak with a smaller product than
    the match already there. The greedy pass rejects the extra match: Y's score has X's bits. Y sits
    at the lower row, X at the earlier position of the caller's list."""
    rng = np.random.default_rng(seed)
    per = []
    for qn in QN:
        q = _query(rng, qn)
        qmz, qint = q[0], q[1]
        picks = rng.choice(qn, min(5, qn), replace=False)
        prods = _split(rng, 0.60, len(picks))
        base = [(int(picks[0]), -0.006, float(prods[0]))] + \
               [(int(i), float(rng.uniform(-0.01, 0.01)), float(p)) for i, p in zip(picks[1:], prods[1:])]
        x = _cand(qmz, qint, base)
        y = _cand(qmz, qint, base + [(int(picks[0]), 0.006, 0.3 * float(prods[0]))])
        cands = _fill(rng, qmz, qint, [], 3, 0.05, 0.30, 0.25)
        cands.append(y)                                                  # local row 3
        _fill(rng, qmz, qint, cands, 20, 0.05, 0.30, 0.25)
        cands.append(x)                                                  # local row 20
        _fill(rng, qmz, qint, cands, N_CAND, 0.05, 0.30, 0.25)
        per.append((q, cands, None))
    return _assemble('c', per, {'y_local': 3, 'x_local': 20})


def case_d(seed=4):
    """Two query peaks closer than the tolerance and every candidate with a peak between them: every
    candidate is deferred, nothing is pruned (there is no exact score to prune against). A query of
    one peak cannot have two: the smallest query of this case has two peaks."""
    rng = np.random.default_rng(seed)
    per = []
    for qn in (2, 37, 100):
        g = _grid(qn - 1)
        at = min(5, qn - 2)
        qmz = np.sort(np.concatenate([g, [np.float32(np.float64(g[at]) + 0.01)]]).astype(np.float32))
        q = (qmz, rng.uniform(0.3, 0.6, qn).astype(np.float32), np.zeros(qn, np.uint8))
        cands = []
        for _ in range(N_CAND):
            mz, it = np.zeros(0, np.float32), np.zeros(0, np.float32)
            if len(g) > 1:
                mz, it, _ = plain(rng, g, q[1], float(rng.uniform(0.1, 0.5)), npk=4, avoid=(at,))
            mid = np.float32(np.float64(g[at]) + 0.005)
            mz2 = np.concatenate([mz, [mid]]).astype(np.float32)
            it2 = np.concatenate([it, [np.float32(0.3)]]).astype(np.float32)
            o = np.argsort(mz2, kind='stable')
            cands.append((mz2[o], it2[o], np.zeros(len(o), np.uint8)))
        per.append((q, cands, None))
    return _assemble('d', per)


def case_e(seed=5, n=1030):
    """A list longer than a super-chunk of the kernels (1024 slots): the deferred candidates are in
    the first super-chunk, the best exact score in the second. Their bounds lie above every exact
    score of the first super-chunk: they are pruned only against the final best."""
    rng = np.random.default_rng(seed)
    q = _query(rng, 37)
    cands = []
    for i in range(n):
        if i == n - 3:
            cands.append(plain(rng, q[0], q[1], 0.60))                  # the winner, slot 1027
        elif i < 1024 and i % 50 == 7:
            cands.append(twin(rng, q[0], q[1], 0.16, 0.01))             # bound ~0.17: above 0.05, below 0.3
        else:
            cands.append(plain(rng, q[0], q[1], float(rng.uniform(0.01, 0.05)), npk=3))
    return _assemble('e', [(q, cands, None)], {'winner_local': n - 3}, order='ascending')


def case_f(seed=6):
    """A query with one negative intensity: a candidate that matches that peak has a negative
    product, its sum of all matches bounds nothing -- deferred, never pruned. (Each such candidate
    matches the peak once, and its total stays positive.)"""
    rng = np.random.default_rng(seed)
    per = []
    for qn in (37, 100):
        qmz, qint, qch = _query(rng, qn)
        qint = qint.copy()
        qint[4] = np.float32(-0.4)
        cands = [plain(rng, qmz, qint, 0.50, avoid=(4,))]               # the winner
        for k in range(1, N_CAND):
            if k % 4 == 1:       # touches the negative peak: product -0.02, total ~0.2 .. 0.4
                mz, it, ch = plain(rng, qmz, qint, float(rng.uniform(0.2, 0.4)), npk=4, avoid=(4,))
                mz2 = np.concatenate([mz, [np.float32(np.float64(qmz[4]) + 0.003)]]).astype(np.float32)
                it2 = np.concatenate([it, [np.float32(0.05)]]).astype(np.float32)
                o = np.argsort(mz2, kind='stable')
                cands.append((mz2[o], it2[o], np.zeros(len(o), np.uint8)))
            else:
                cands.append(plain(rng, qmz, qint, float(rng.uniform(0.05, 0.45)), avoid=(4,)))
        per.append(((qmz, qint, qch), cands, None))
    return _assemble('f', per)


CASES = {'a': case_a, 'b': case_b, 'c': case_c, 'd': case_d, 'e': case_e, 'f': case_f}
_CACHE = {}


def get(name):
    """The case, built once per process and shared (callers must not modify it)."""
    if name not in _CACHE:
        _CACHE[name] = CASES[name]()
    return _CACHE[name]


# ------------------------------------------------------------------ what the kernels must count
def pair_facts(case, qi, row):
    """(bound, deferred, prunable-by-sign) of the pair (query qi, library row): from match_list."""
    qo, qmz, qit, _, qpmz, _ = case.queries
    lo, lmz, lit, lch, lpmz, lz = case.library
    a, b = slice(qo[qi], qo[qi + 1]), slice(lo[row], lo[row + 1])
    m = match_list(qmz[a], qit[a], qpmz[qi], lmz[b], lit[b], lch[b], lpmz[row], int(lz[row]), TOL, True)
    total, repeats, signed = bound_of(m)
    return total, repeats or signed, not signed


def expected_counts(O, case):
    """Per query (deferred, pruned, [(row, bound, exact score, deferred, pruned)]): a candidate is
    deferred when a peak repeats among its generated matches (or a product is negative), and pruned
    when its bound, with the kernels' slack, lies below the best exact score among the query's
    candidates that are not deferred. Exact scores are the oracle's."""
    Q, L = O.Spectra(*case.queries), O.Spectra(*case.library)
    out = []
    for qi, rows in enumerate(case.lists):
        info, best = [], 0.0
        for r in rows:
            bound, deferred, has_bound = pair_facts(case, qi, int(r))
            _, s, _ = O.best_match(Q, qi, L, np.array([r], np.int64), TOL, True)
            info.append([int(r), bound, s, deferred, has_bound])
            if not deferred:
                best = max(best, s)
        rec = []
        for r, bound, s, deferred, has_bound in info:
            pruned = deferred and has_bound and bound * (1.0 + PRUNE_REL) + PRUNE_ABS < best
            rec.append((r, bound, s, deferred, pruned))
        out.append((sum(x[3] for x in rec), sum(x[4] for x in rec), rec, best))
    return out
