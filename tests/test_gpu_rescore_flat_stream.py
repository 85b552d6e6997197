"""The flat rescoring kernel's stream of candidate peaks (csrc/rescore.hip, rescore_flat_kernel): a
wave sets 32 candidates up at a time, walks their peaks as one stream of 64 per step -- a stream
position's candidate comes from an owner table, the candidate's peak record and key from two small
per-candidate tables -- queues the (peak, shift) items whose bin is marked and scores them a row of
64 at a time.

Planted here are the shapes at which that bookkeeping can go wrong: list lengths around the chunk of
32 and the four waves of a query; chunks whose peak counts end at and around the owner table's
1 024; candidates that own no stream position (more than 64 peaks, precursor charge >= 5, a mass
difference beyond the filter's envelope) at the first and the last lane and in runs; a step in which
every lane hits at every shift, queues of exactly 128 and 129 items; precursor charges 1 - 4 in one
chunk, one and no charge-3 candidate (the fp64 division's guard), annotated peaks, no shifts; slot
lists longer than a super-chunk with invalid slots at its edges, and one that is split over blocks.

Through asl_rescore_batch (FORM 0), asl_rescore_knn (FORM 2), the ANN search with the scan-side
filter (FORM 1) and a window-only search (FORM 3); winner-only and ranked (n = 5), in Da and in ppm.
Every comparison with the oracle is exact -- winner, score bits, match count, match list -- and
`_every_candidate` makes each candidate of a list the winner in turn, so that a score that moved in
a losing candidate is seen. The kernels' counters (deferred, pruned, work-list items) are held
against a CPU count."""
import numpy as np
import pytest

import ppm_ref
import prune_cases as PC
import rescore_cases as RC
from test_gpu_rescore_prune import _Counted, _items

pytestmark = pytest.mark.gpu

TOL = 0.02
QPMZ = 650.0
PMD = 3.0                   # shifts 3, 1.5, 1, 0.75 Da: off the queries' 10 Da grid


# ------------------------------------------------------------------ planting
def _cand(rng, q, npk, z=2, pmd=0.0, nhit=5, twin=False, annotate=False):
    """A candidate of npk peaks: nhit of them in the windows of distinct query peaks, each at one of
    the shifts its precursor charge gives (at most the four the flat kernel's table holds), the others
    half-way between the grid points (they match at no shift). twin: a second peak in the first
    window, at the same shift (a doubly matched query peak). annotate: a shifted peak carries its
    shift as fragment charge, an unshifted one a random charge."""
    qmz = q[0]
    ns = z + 1 if abs(pmd) >= TOL else 1
    nhit = min(nhit, npk - (1 if twin else 0), len(qmz))
    picks = rng.choice(len(qmz), nhit, replace=False)
    pos, chg = [], []
    for k, i in enumerate(picks):
        s = int(rng.integers(0, min(ns, 5)))
        off = -0.006 if (twin and k == 0) else float(rng.uniform(-0.008, 0.008))
        pos.append(float(qmz[i]) + off - (pmd / s if s else 0.0))
        chg.append((s if s else int(rng.integers(0, z + 1))) if annotate else 0)
        if twin and k == 0:
            pos.append(pos[-1] + 0.012)
            chg.append(chg[-1])
    slots = rng.choice(150, npk - len(pos), replace=False)
    pos += [205.0 + 10.0 * int(k) + float(rng.uniform(-1.0, 1.0)) for k in slots]
    chg += [0] * len(slots)
    mz = np.array(pos, np.float64).astype(np.float32)
    order = np.argsort(mz, kind='stable')
    assert np.all(np.diff(mz[order]) > 0) and mz.min() > 0
    return mz[order], rng.uniform(0.3, 0.6, npk).astype(np.float32), np.array(chg, np.uint8)[order]


class World:
    """Queries with a list of candidates each; a candidate is (spectrum, precursor charge, pmd)."""

    def __init__(self, name):
        self.name, self.qs, self.lib, self.l_pmz, self.l_z, self.lists = name, [], [], [], [], []

    def add(self, q, cands, invalid=(), repeat=1):
        base = len(self.lib)
        for spec, z, pmd in cands:
            self.lib.append(spec)
            self.l_z.append(z)
            self.l_pmz.append(QPMZ - pmd / z)
        rows = np.tile(np.arange(base, base + len(cands), dtype=np.int64), repeat)
        rows[list(invalid)] = -1
        self.qs.append(q)
        self.lists.append(rows)
        return self

    def case(self):
        n = len(self.qs)
        return PC.Case(self.name, RC.pack(self.qs, [QPMZ] * n, [2] * n), RC.pack(self.lib, self.l_pmz, self.l_z),
                       self.lists)


def _plain_list(rng, q, n, every_twin=7):
    return [(_cand(rng, q, int(rng.integers(5, 31)), 2, PMD if k % 2 else 0.0, twin=(k % every_twin == 3)), 2,
             PMD if k % 2 else 0.0) for k in range(n)]


def _per_wave(pattern):
    """The same candidates for each of the four waves of a query's block."""
    return [c for _ in range(4) for c in pattern]


# ------------------------------------------------------------------ what the kernels must give
def _facts(case, qi, row, shift, O):
    """(route, bound, deferred, has_bound, exact score) of a pair; cached in the case."""
    _FACTS = case.notes.setdefault('facts', {})
    key = (qi, row, shift)
    if key not in _FACTS:
        qo, qmz, qit, _, qpmz, _ = case.queries
        lo, lmz, lit, lch, lpmz, lz = case.library
        a, b = slice(qo[qi], qo[qi + 1]), slice(lo[row], lo[row + 1])
        z, cn = int(lz[row]), int(lo[row + 1] - lo[row])
        pmd = (float(qpmz[qi]) - float(lpmz[row])) * z
        S = z + 1 if (shift and abs(pmd) >= TOL) else 1
        route = 'bs' if (cn > 64 or z >= 31 or (S > 1 and not abs(pmd) <= RC.RS_MD_ENV)) else 'pair' if S > 5 else 'flat'
        m = PC.match_list(qmz[a], qit[a], qpmz[qi], lmz[b], lit[b], lch[b], lpmz[row], z, TOL, shift)
        total, repeats, signed = PC.bound_of(m)
        _, s, _ = O.best_match(O.Spectra(*case.queries), qi, O.Spectra(*case.library), np.array([row], np.int64), TOL,
                               shift)
        _FACTS[key] = (route, total, repeats or signed, not signed, s)
    return _FACTS[key]


def _expected_counts(O, case, shift=True, prune=True):
    deferred = pruned = items = 0
    for qi, rows in enumerate(case.lists):
        f = [_facts(case, qi, int(r), shift, O) for r in rows if r >= 0]
        best = max([x[4] for x in f if x[0] == 'flat' and not x[2]], default=0.0)
        d = sum(x[0] == 'pair' or (x[0] == 'flat' and x[2]) for x in f)
        p = sum(x[0] == 'flat' and x[2] and x[3] and x[1] * (1.0 + PC.PRUNE_REL) + PC.PRUNE_ABS < best
                for x in f) if prune else 0
        deferred, pruned, items = deferred + d, pruned + p, items + _items(d - p)
    return deferred, pruned, items


def _oracle_best(O, Q, L, qi, rows, shift):
    pos = np.nonzero(rows >= 0)[0]
    b, s, m = O.best_match(Q, qi, L, rows[pos], TOL, shift)
    return int(pos[b]), s, m


def _check_batch(O, case, shift=True, prune=True, ranked=True):
    """asl_rescore_batch (FORM 0): winner, score, matches and counters; then the ranked request."""
    from ann_solo_amd import spectrum_match
    from test_gpu_topn import _check_query, _oracle_ranks
    q, lib = case.packed()
    rows, off = case.csr()
    with _Counted() as cnt:
        best, score, count, pairs = spectrum_match.rescore_batch(q, lib, rows, off, TOL, shift)
    Q, L = O.Spectra(*case.queries), O.Spectra(*case.library)
    for qi in range(case.nq):
        b, s, m = _oracle_best(O, Q, L, qi, case.lists[qi], shift)
        assert best[qi] == b, (case.name, qi, int(best[qi]), b)
        assert score[qi] == s and count[qi] == len(m), (case.name, qi, float(score[qi]), s)
        assert pairs[qi, :len(m)].tolist() == m.tolist(), (case.name, qi)
    want = _expected_counts(O, case, shift, prune)
    print('%s: deferred %d pruned %d items %d (CPU count %r)' % (case.name, cnt.deferred, cnt.pruned, cnt.items, want))
    assert (cnt.deferred, cnt.pruned, cnt.items) == want, case.name
    if ranked:
        with _Counted() as cnt:
            top = spectrum_match.rescore_batch_topn(q, lib, rows, off, TOL, shift, 5)
        for qi in range(case.nq):
            pos = np.nonzero(case.lists[qi] >= 0)[0]
            ranks = _oracle_ranks(O, Q, qi, L, case.lists[qi][pos], 5, TOL, shift)
            _check_query(top[0][qi], top[1][qi], top[2][qi], top[3][qi], [(int(pos[p]), s, m) for p, _, s, m in ranks],
                         5, (case.name, qi))
        assert cnt.pruned == 0 and cnt.deferred == want[0], case.name


def _every_candidate(O, case, qi=0, shift=True):
    """Query qi's list once per candidate, in a library in which that candidate's intensities are 64
    times as large: same peak counts, shifts and chunks, and every candidate's score is a winner's."""
    from ann_solo_amd import spectrum_match
    from ann_solo_amd.packed import PackedSpectra
    qo, qmz, qit, qch, qpmz, qz = case.queries
    lo, lmz, lit, lch, lpmz, lz = case.library
    rows = case.lists[qi]
    n = len(rows)
    spec = lambda r, f: (lmz[lo[r]:lo[r + 1]], lit[lo[r]:lo[r + 1]] * np.float32(f), lch[lo[r]:lo[r + 1]])
    lib, pmz, zs = [], [], []
    for i in range(n):
        lib += [spec(r, 64.0 if k == i else 1.0) for k, r in enumerate(rows)]
        pmz += [lpmz[r] for r in rows]
        zs += [lz[r] for r in rows]
    a = slice(qo[qi], qo[qi + 1])
    queries = RC.pack([(qmz[a], qit[a], qch[a])] * n, [qpmz[qi]] * n, [qz[qi]] * n)
    library = RC.pack(lib, pmz, zs)
    cand = np.arange(n * n, dtype=np.int64)
    off = (np.arange(n + 1) * n).astype(np.int32)
    best, score, count, pairs = spectrum_match.rescore_batch(
        PackedSpectra.from_numpy(*queries), PackedSpectra.from_numpy(*library), cand, off, TOL, shift)
    Q, L = O.Spectra(*queries), O.Spectra(*library)
    winners = set()
    for i in range(n):
        b, s, m = O.best_match(Q, i, L, cand[off[i]:off[i + 1]], TOL, shift)
        assert best[i] == b and score[i] == s and count[i] == len(m), (case.name, i, int(best[i]), b, float(score[i]), s)
        assert pairs[i, :len(m)].tolist() == m.tolist(), (case.name, i)
        winners.add(b)
    return len(winners)


# ------------------------------------------------------------------ list lengths
def test_candidates_per_query(O):
    """1 .. 133 candidates: one lane, one per wave, a wave with two, a chunk less one, full, plus one,
    and four waves' chunks less one, full, plus one, plus five."""
    rng = np.random.default_rng(101)
    w = World('lengths')
    for n in (1, 4, 5, 31, 32, 33, 127, 128, 129, 133):
        q = PC._query(rng, 37)
        w.add(q, _plain_list(rng, q, n))
    case = w.case()
    _check_batch(O, case)
    for qi in (1, 2, 5):              # 4, 5 and 33 candidates: every one of them
        assert _every_candidate(O, case, qi) >= len(case.lists[qi]) - 1


# ------------------------------------------------------------------ peak counts of a chunk
PATTERNS = {
    'ends_1023': [64] * 15 + [63] + [7] * 3,
    'ends_1024': [64] * 15 + [63, 1] + [7] * 3,
    'ends_1025': [64] * 15 + [63, 2] + [7] * 3,         # the 17th candidate opens the next chunk
    '16x64': [64] * 16,
    '17x64': [64] * 17,
    '32x1': [1] * 32,
    'stream_1': [1],
    'stream_63': [63],
    'stream_64': [64],
    'stream_65': [64, 1],
    'stream_128': [64, 64],
}


@pytest.mark.parametrize('group', [('ends_1023', 'ends_1024', 'ends_1025'), ('16x64', '17x64'),
                                   ('32x1', 'stream_1', 'stream_63', 'stream_64', 'stream_65', 'stream_128')])
def test_peak_counts_of_a_chunk(O, group):
    rng = np.random.default_rng(102)
    w = World('+'.join(group))
    for name in group:
        q = PC._query(rng, 100)
        pattern = [(_cand(rng, q, npk, 2, PMD if k % 3 else 0.0, nhit=min(npk, 6), twin=(npk > 8 and k % 5 == 2)), 2,
                    PMD if k % 3 else 0.0) for k, npk in enumerate(PATTERNS[name])]
        w.add(q, _per_wave(pattern))
    case = w.case()
    _check_batch(O, case)
    for qi, name in enumerate(group):
        if name in ('ends_1024', 'ends_1025', '17x64', '32x1', 'stream_65'):
            assert _every_candidate(O, case, qi) >= 4


# ------------------------------------------------------------------ candidates without a stream position
def test_candidates_that_own_no_stream_position(O):
    """More than 64 peaks and a mass difference beyond the envelope go to the binary-search kernel,
    precursor charge 5 with a shift to the pair kernel: at lane 0, at lane 31 and in a run between
    ordinary candidates, whose scores must not move."""
    rng = np.random.default_rng(103)
    q = PC._query(rng, 37)
    big = lambda: (_cand(rng, q, 70, 2, PMD, nhit=8), 2, PMD)
    z5 = lambda: (_cand(rng, q, 12, 5, PMD), 5, PMD)
    env = lambda: (_cand(rng, q, 12, 2, -5000.0), 2, -5000.0)
    pattern = _plain_list(rng, q, 32)
    pattern[0], pattern[31] = big(), z5()
    pattern[10:14] = [env(), big(), z5(), env()]
    w = World('no_position').add(q, _per_wave(pattern))
    q2 = PC._query(rng, 37)           # a chunk of nothing else, and one ordinary candidate among them
    w.add(q2, _per_wave([(_cand(rng, q2, 66, 2, 0.0), 2, 0.0), (_cand(rng, q2, 9, 6, PMD), 6, PMD)] * 4))
    w.add(q2, _per_wave([(_cand(rng, q2, 66, 2, 0.0), 2, 0.0)] * 3 + [(_cand(rng, q2, 9, 2, PMD), 2, PMD)] +
                        [(_cand(rng, q2, 9, 6, PMD), 6, PMD)] * 3))
    case = w.case()
    _check_batch(O, case)
    pattern_case = World('no_position_one_wave').add(q, pattern).case()      # 8 candidates per wave
    assert _every_candidate(O, pattern_case) >= 30


# ------------------------------------------------------------------ the queue
def _ladder(rng, step, n_peaks, first=0):
    """Query: 100 peaks `step` Da apart. Candidate (charge 2, pmd = 3: shifts of 3 and 1.5 Da): n_peaks
    peaks on that ladder, every one in a window at shift 0 and at each shift that is a multiple of
    the step."""
    qmz = (200.0 + step * np.arange(100)).astype(np.float32)
    q = (qmz, rng.uniform(0.3, 0.6, 100).astype(np.float32), np.zeros(100, np.uint8))
    c = (qmz[first:first + n_peaks].copy(), rng.uniform(0.3, 0.6, n_peaks).astype(np.float32),
         np.zeros(n_peaks, np.uint8))
    return q, (c, 2, PMD)


def test_queue_sizes(O):
    """All 64 lanes of a step hit at all three shifts (192 items: a drain inside the step); a chunk
    that queues exactly 128 items, and one with 129. The queue's length is arranged, not observed:
    asserted is the number of generated matches of the ladder candidate, which is the number of queued
    items as long as the bin bitmap marks no bin of the shift that matches nothing (the ladders stay
    within 300 Da, far below the bitmap's period of 655.36 Da, and 1.5 Da off every query peak)."""
    rng = np.random.default_rng(104)
    w = World('queue')
    q, c = _ladder(rng, 1.5, 64)
    w.add(q, _per_wave([c]))
    q, c = _ladder(rng, 3.0, 64)                    # shifts 0 and 1 (3 Da) hit, shift 2 (1.5 Da) does not
    w.add(q, _per_wave([c]))
    one = ((np.array([q[0][70]], np.float32), np.array([0.5], np.float32), np.zeros(1, np.uint8)), 2, 0.0)
    w.add(q, _per_wave([c, one]))
    w.add(q, _per_wave([one, c]))
    case = w.case()
    qo, qmz, qit = case.queries[:3]
    lo, lmz, lit, lch, lpmz, lz = case.library
    for qi, (slot, items) in enumerate(((0, 192), (0, 128), (0, 128), (1, 128))):     # the ladder candidate's matches
        r = int(case.lists[qi][slot])
        a, b = slice(qo[qi], qo[qi + 1]), slice(lo[r], lo[r + 1])
        m = PC.match_list(qmz[a], qit[a], QPMZ, lmz[b], lit[b], lch[b], lpmz[r], 2, TOL, True)
        assert len(m) == items, (qi, len(m))
    _check_batch(O, case)


# ------------------------------------------------------------------ charges
@pytest.mark.parametrize('mix', ['1234', 'one_3', 'no_3', 'annotated'])
def test_charge_mixes(O, mix):
    """Precursor charges 1 - 4 in one chunk (two to five shifts; the shift table's third entry needs an
    fp64 division, done only where a chunk holds a candidate of charge >= 3); exactly one charge-3
    candidate among charge-2 ones, at lane 17; none; annotated peaks."""
    rng = np.random.default_rng(105)
    q = PC._query(rng, 37)
    zs = {'1234': [1 + k % 4 for k in range(32)], 'one_3': [3 if k == 17 else 2 for k in range(32)],
          'no_3': [2 if k % 2 else 1 for k in range(32)], 'annotated': [1 + k % 4 for k in range(32)]}[mix]
    pattern = [(_cand(rng, q, int(rng.integers(6, 40)), z, PMD, nhit=6, twin=(k % 6 == 1), annotate=(mix == 'annotated')),
                z, PMD) for k, z in enumerate(zs)]
    case = World('charges_' + mix).add(q, _per_wave(pattern)).case()
    _check_batch(O, case)
    one_wave = World('charges_' + mix + '_one_wave').add(q, pattern).case()
    assert _every_candidate(O, one_wave) >= 30
    # no shifts: the same lists with allow_shift off
    _check_batch(O, case, shift=False, ranked=False)


# ------------------------------------------------------------------ long slot lists
def test_lists_longer_than_a_super_chunk(O):
    """1 025 and 2 049 slots with invalid slots at the first, a middle and the last position of a
    super-chunk of 1 024; the winner sits behind the last boundary."""
    rng = np.random.default_rng(106)
    w = World('long')
    for n, bad in ((1025, (0, 512, 1023)), (2049, (0, 1023, 1024, 1536, 2047))):
        q = PC._query(rng, 37)
        pool = _plain_list(rng, q, 41, every_twin=20)     # (fewer deferred candidates than the kernel's list holds)
        pool[(n - 1) % 41] = (PC.plain(rng, q[0], q[1], 4.0, npk=5), 2, 0.0)      # the last slot's row: the best
        w.add(q, pool, invalid=bad, repeat=n // 41 + 1)
        w.lists[-1] = w.lists[-1][:n]
    case = w.case()
    assert [len(x) for x in case.lists] == [1025, 2049]
    _check_batch(O, case)


def test_list_split_over_blocks(O):
    """One query with 5 000 slots: its list is split over several blocks, which switches pruning off
    (no block sees every exact score) and leaves the work list to its own kernel."""
    rng = np.random.default_rng(107)
    q = PC._query(rng, 37)
    w = World('split').add(q, _plain_list(rng, q, 97), invalid=(0, 4999), repeat=52)
    w.lists[-1] = w.lists[-1][:5000]
    _check_batch(O, w.case(), prune=False)


# ------------------------------------------------------------------ the packed-record forms
def _charge2_world(rng, nq=6, n=40):
    w = World('shaped')
    for _ in range(nq):
        q = PC._query(rng, 37)
        c = _plain_list(rng, q, n)
        c[0] = (_cand(rng, q, 70, 2, PMD, nhit=8), 2, PMD)                 # no stream position, first lane
        c[7] = (_cand(rng, q, 12, 2, -5000.0), 2, -5000.0)
        w.add(q, c)
    return w.case()


def test_rescore_knn_form(O):
    """FORM 2 (asl_rescore_knn over an asl_library_t: row records and peak records), lists of 40 with
    two empty slots; ties go to the lowest row."""
    import torch
    from ann_solo_amd.distributed import HipShardBackend
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    case = _charge2_world(np.random.default_rng(108))
    q, lib = case.packed()
    K = 42
    cfg = Config.open_search(num_list=1 << 20, num_candidates=K, fragment_mz_tolerance=TOL,
                             precursor_tolerance_mass_open=1e12, precursor_tolerance_mode_open='Da')
    sl = SpectralLibrary(lib, config=cfg)
    try:
        part = sl.partitions[2]
        assert part.spectra.n == lib.n
        knn = np.full((case.nq, K), -1, np.int64)
        for qi, rows in enumerate(case.lists):
            knn[qi, 1:1 + len(rows)] = rows[::-1]
        with _Counted() as cnt:
            res = HipShardBackend(sl, 2, 'open').rescore_knn(q, torch.from_numpy(knn).to(sl.device))
        Q, P = O.Spectra(*case.queries), O.Spectra(*part.spectra.to('cpu').numpy())
        for qi in range(case.nq):
            cand = np.sort(case.lists[qi])
            b, s, m = O.best_match(Q, qi, P, cand, TOL, True)
            assert res.n_candidates[qi] == len(cand) and res.best_row[qi] == cand[b], (qi, int(res.best_row[qi]))
            assert res.best_score[qi] == s and res.pm_count[qi] == len(m), (qi, float(res.best_score[qi]), s)
            assert res.pm_pairs[qi, :len(m)].tolist() == m.tolist(), qi
        assert (cnt.deferred, cnt.pruned, cnt.items) == _expected_counts(O, case)
    finally:
        sl.shutdown()


def test_window_only_form(O):
    """FORM 3: a window-only search; every library row is in every query's window (240 candidates a
    query, the other queries' among them)."""
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    base = _charge2_world(np.random.default_rng(109))
    q, lib = base.packed()
    every = np.arange(lib.n, dtype=np.int64)
    case = PC.Case('window', base.queries, base.library, [every] * base.nq)
    cfg = Config.open_search(mode='bf', fragment_mz_tolerance=TOL, precursor_tolerance_mass=20,
                             precursor_tolerance_mode='ppm', precursor_tolerance_mass_open=10000,     # (holds |pmd| = 5 000)
                             precursor_tolerance_mode_open='Da')
    sl = SpectralLibrary(lib, config=cfg)
    try:
        part = sl.partitions[2]
        assert part.spectra.n == lib.n
        with _Counted() as cnt:
            res = sl._search_batch(q, 2, 'open')
        Q, P = O.Spectra(*base.queries), O.Spectra(*part.spectra.to('cpu').numpy())
        for qi in range(base.nq):
            b, s, m = O.best_match(Q, qi, P, every, TOL, True)
            assert res.n_candidates[qi] == lib.n and res.best_row[qi] == every[b], qi
            assert res.best_score[qi] == s and res.pm_count[qi] == len(m), qi
            assert res.pm_pairs[qi, :len(m)].tolist() == m.tolist(), qi
        assert (cnt.deferred, cnt.pruned, cnt.items) == _expected_counts(O, case)
    finally:
        sl.shutdown()


@pytest.mark.parametrize('nq', [97, 129])
def test_ann_search_form(O, nq):
    """FORM 1: the ANN search's own lists, filtered in the scan, winner-only and ranked (n = 5), at
    batch sizes that are no multiple of anything."""
    from ann_solo_amd import synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    from test_gpu_topn import _check_open, _consistent, _postfilter
    lib, aux = synthetic.make_library(3000, seed=110, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, nq, seed=111, charge=2)
    tol, mode = 250.0, 'Da'
    cfg = Config.open_search(num_list=16, num_probe=8, num_candidates=133, index='ivfpq', kmeans_niter=4,
                             precursor_tolerance_mass_open=tol, precursor_tolerance_mode_open=mode)
    sl = SpectralLibrary(lib, config=cfg)
    prev = _postfilter(1)
    try:
        top = sl.search_batch_topn(q, 2, 'open', 5, want_knn=True)
        _check_open(O, sl, q, 2, tol, mode, top, 5, ('ann', nq))
        _consistent(top, sl._search_batch(q, 2, 'open', want_knn=True), 5, what=('ann', nq))
    finally:
        _postfilter(prev)
        sl.shutdown()


# ------------------------------------------------------------------ ppm
def test_ppm_winner_and_ranked():
    """The same kind of lists with the fragment tolerance in ppm (40 ppm: 0.008 - 0.023 Da over the
    queries' range), winner-only and ranked, against the ppm reference."""
    from ann_solo_amd import spectrum_match
    rng = np.random.default_rng(112)
    w = World('ppm')
    for n in (5, 33, 40):
        q = PC._query(rng, 37)
        w.add(q, [(_cand(rng, q, int(rng.integers(5, 31)), 1 + k % 4, PMD, twin=(k % 7 == 3)), 1 + k % 4, PMD)
                  for k in range(n)])
    case = w.case()
    q, lib = case.packed()
    rows, off = case.csr()
    best, score, count, pairs = spectrum_match.rescore_batch(q, lib, rows, off, 40.0, True,
                                                             fragment_tolerance_unit='ppm')
    top = spectrum_match.rescore_batch_topn(q, lib, rows, off, 40.0, True, 5, fragment_tolerance_unit='ppm')
    for qi in range(case.nq):
        sc = ppm_ref.scores(case.queries, qi, case.library, case.lists[qi], 40.0, True, 'ppm')
        order = ppm_ref.ranked(sc, 5)
        b, s, m = ppm_ref.best_match(case.queries, qi, case.library, case.lists[qi], 40.0, True, 'ppm')
        assert best[qi] == b == order[0] and score[qi] == s and count[qi] == len(m), (qi, float(score[qi]), s)
        assert pairs[qi, :len(m)].tolist() == m.tolist(), qi
        assert top[0][qi].tolist() == order.tolist(), qi
        assert top[1][qi].tolist() == sc[order].tolist(), qi
