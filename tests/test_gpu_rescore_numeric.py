"""The rescoring's two analytic bounds, against the oracle (csrc/rescore.hip):

* the fp32 bin filter of the flat and the pair kernel -- a shifted candidate peak's bin is computed
  in fp32 and the query peaks are filed with a margin that has to cover its rounding; a match the
  filter drops is lost silently. tests/rescore_cases.py plants candidate peaks on the window edges
  inside the filter's envelope, at its routing threshold, and beyond it by fragment m/z and by
  precursor mass difference (regimes 1 .. 5; tests/test_rescore_cases_cpu.py counts what is planted);
* the exact-sum gate -- products are added in arrival order and the sum is kept only while their
  exponents span <= 23 binades; and products that are denormal, zero or near the top of the float
  range, where ties go by generation order.

Every comparison is exact: score bits, match count and match list of every pair."""
import numpy as np
import pytest

import rescore_cases as RC

pytestmark = pytest.mark.gpu


def _packed(t):
    from ann_solo_amd.packed import PackedSpectra
    return PackedSpectra.from_numpy(*t)


def _pairs_one_to_one(O, queries, library, owner, tol, shift=True):
    """Every (owner[r], r) pair as a candidate list of length one: score, match count and match list
    against the oracle. Returns the list of mismatching rows (with what differed)."""
    from ann_solo_amd import spectrum_match
    owner = np.asarray(owner, np.int64)
    lib = _packed(library)
    q = _packed(queries).select(owner)                    # one query entry per pair
    n = lib.n
    best, score, count, pairs = spectrum_match.rescore_batch(
        q, lib, np.arange(n, dtype=np.int64), np.arange(n + 1, dtype=np.int32), tol, shift)
    L, Q = O.Spectra(*library), O.Spectra(*queries)
    bad = []
    for r in range(n):
        b, s, m = O.best_match(Q, int(owner[r]), L, np.array([r], np.int64), tol, shift)
        assert b == 0
        if best[r] != 0:
            bad.append((r, 'no winner'))
        elif score[r] != s:
            bad.append((r, 'score %r != %r (matches %d / %d)' % (float(score[r]), s, int(count[r]), len(m))))
        elif count[r] != len(m):
            bad.append((r, 'count %d != %d' % (int(count[r]), len(m))))
        elif pairs[r, :len(m)].tolist() != m.tolist():
            bad.append((r, 'match list'))
    return bad


def _report(failed):
    return '\n'.join('%s: %d of %d differ, e.g. %d: %s' % (name, k, n, r, what)
                     for name, k, n, (r, what) in failed)


@pytest.mark.parametrize('number', RC.REGIMES)
def test_regime_one_candidate_lists(O, number):
    """Every planted pair on its own: a winner-only check over long lists would hide a lost match
    in a losing candidate."""
    failed = []
    for block in RC.regime_blocks(number):
        bad = _pairs_one_to_one(O, block.queries, block.library, block.owner, block.tol)
        print('%s: %d of %d pairs differ' % (block.name, len(bad), block.nlib))
        if bad:
            failed.append((block.name, len(bad), block.nlib, bad[0]))
    assert not failed, _report(failed)


@pytest.mark.parametrize('number', RC.REGIMES)
def test_regime_grouped_lists(O, number):
    """The same pairs in lists of 40 per query (full 32-candidate wave chunks and a second chunk):
    winner, score and matches."""
    from ann_solo_amd import spectrum_match
    failed = []
    for block in RC.regime_blocks(number):
        q, lib = block.packed()
        rows, off = RC.grouped_lists(block)
        best, score, count, pairs = spectrum_match.rescore_batch(q, lib, rows, off, block.tol, True)
        L, Q = O.Spectra(*block.library), O.Spectra(*block.queries)
        bad = []
        for qi in range(block.nq):
            b, s, m = O.best_match(Q, qi, L, rows[off[qi]:off[qi + 1]], block.tol, True)
            if best[qi] != b:
                bad.append((qi, 'winner %d != %d' % (int(best[qi]), b)))
            elif score[qi] != s or count[qi] != len(m) or pairs[qi, :len(m)].tolist() != m.tolist():
                bad.append((qi, 'score %r != %r or matches (%d / %d)' % (float(score[qi]), s, int(count[qi]), len(m))))
        print('%s: %d of %d queries differ' % (block.name, len(bad), block.nq))
        if bad:
            failed.append((block.name, len(bad), block.nq, bad[0]))
    assert not failed, _report(failed)


@pytest.mark.parametrize('number', [1, 4, 5])
def test_regime_shaped_path(O, number):
    """The packed-record path (asl_rescore_knn over an asl_library_t, through the engine's
    rescore_knn): the flat kernel reads row records and peak records there. asl_rescore_knn takes
    int64 neighbour lists only, so this is the kernels' FORM 2; the int32 form (FORM 1: the fused
    search's own lists) differs in the width of the row load alone. One library handle per
    precursor charge; a query's fixed-stride list holds its own candidates of that charge and
    others', the rest of the row is -1."""
    import torch
    from ann_solo_amd.distributed import HipShardBackend
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    K = 40
    failed = []
    for block in RC.regime_blocks(number):
        q, lib = block.packed()
        cfg = Config.open_search(num_list=1 << 20, num_candidates=K, fragment_mz_tolerance=block.tol,
                                 precursor_tolerance_mass_open=1e12, precursor_tolerance_mode_open='Da')
        sl = SpectralLibrary(lib, config=cfg)
        try:
            lz = block.library[5]
            Q = O.Spectra(*block.queries)
            bad, total = [], 0
            for z, part in sorted(sl.partitions.items()):
                glob = np.nonzero(lz == z)[0]                       # partition row -> library row
                own = block.owner[glob]
                knn = np.full((block.nq, K), -1, np.int64)
                for qi in range(block.nq):
                    mine, other = np.nonzero(own == qi)[0], np.nonzero(own != qi)[0]
                    take = np.concatenate([mine, np.roll(other, -3 * qi)])[:K - 2]   # (two slots stay -1)
                    knn[qi, :len(take)] = take
                res = HipShardBackend(sl, int(z), 'open').rescore_knn(
                    q, torch.from_numpy(knn).to(sl.device))
                P = O.Spectra(*part.spectra.to('cpu').numpy())
                for qi in range(block.nq):
                    cand = np.sort(knn[qi][knn[qi] >= 0])           # ties go to the lowest row
                    b, s, m = O.best_match(Q, qi, P, cand, block.tol, True)
                    total += 1
                    if res.n_candidates[qi] != len(cand) or res.best_row[qi] != cand[b]:
                        bad.append((qi, 'z %d: winner %d != %d' % (z, int(res.best_row[qi]), int(cand[b]))))
                    elif (res.best_score[qi] != s or res.pm_count[qi] != len(m) or
                          res.pm_pairs[qi, :len(m)].tolist() != m.tolist()):
                        bad.append((qi, 'z %d: score %r != %r or matches' % (z, float(res.best_score[qi]), s)))
            print('%s: %d of %d lists differ' % (block.name, len(bad), total))
            if bad:
                failed.append((block.name, len(bad), total, bad[0]))
        finally:
            sl.shutdown()
    assert not failed, _report(failed)


# ------------------------------------------------------------------ exact-sum gate
@pytest.mark.parametrize('shifted', [False, True])
def test_exact_sum_gate(O, shifted):
    """Exponent spreads 22 / 23 (the unordered sum is exact: 24 + 23 + 6 = 53 bits) and 24 / 25 / 40
    (it is not: sort and greedy pass), with 64 and with 32 matches, one and several small products
    (tests/rescore_cases.py: gate_case; test_rescore_cases_cpu.py shows that at spread 24 an
    arrival order exists whose sum differs), in every kernel that sums: precursor charge 31 goes to the
    binary-search kernel; charge 5 reaches the pair kernel in the shifted variant only (unshifted,
    pmd = 0 leaves one shift and charges 2 and 5 both stay in the flat kernel, which hands the
    spreads above 23 to the pair kernel's sort). Bit-equal to the sorted-order sum."""
    queries, library, owner, meta = RC.gate_case(shifted)
    L, Q = O.Spectra(*library), O.Spectra(*queries)
    for r in range(0, len(owner), 7):      # the oracle's score IS the sum in descending order
        _, s, m = O.best_match(Q, int(owner[r]), L, np.array([r], np.int64), 0.02, True)
        p = RC.gate_products(library, r, shifted)
        assert s == RC.sum_in_order(np.sort(p)[::-1]) and len(m) == meta[r][0]
    bad = _pairs_one_to_one(O, queries, library, owner, 0.02)
    assert not bad, '%d of %d pairs differ, e.g. %r %r' % (len(bad), len(owner), bad[0], meta[bad[0][0]])


# ------------------------------------------------------------------ product range
def _range_case(kind, z, rng):
    """41 query peaks 10 Da apart plus one at (peak 5) + 3 Da; the candidate (pmd = 3 Da) has a peak
    on every query peak. Candidate peak 5 matches query peak 5 unshifted and the extra query peak at
    shift 1: a positive and a ZERO product compete for it (the extra peak's intensity is 0, or
    query peak 5's). Twins: a second candidate peak inside the windows of query peaks 7, 8, 20."""
    n = 41
    qmz = (200.0 + 10.0 * np.arange(n)).astype(np.float32)
    cmz = qmz.copy()
    if kind == 'denormal':            # products 1e-45 .. 1e-38
        qi_, ci_ = np.full(n, 1e-20), 10.0 ** rng.uniform(-25, -18, n)
    elif kind == 'underflow':         # half of the products round to 0
        qi_, ci_ = np.where(np.arange(n) % 2, 1e-30, 1.0), 10.0 ** rng.uniform(-30, -20, n)
    elif kind == 'zero':              # intensities exactly 0 on both sides
        qi_, ci_ = rng.lognormal(0, 1, n), rng.lognormal(0, 1, n)
        qi_[rng.choice(n, n // 3, replace=False)] = 0.0
        ci_[rng.choice(n, n // 3, replace=False)] = 0.0
    elif kind == 'huge':              # products near 1e38
        qi_, ci_ = np.full(n, 1e19), 10.0 ** rng.uniform(18, 19, n)
    elif kind == 'equal':             # every product the same: ties by generation order
        qi_, ci_ = np.full(n, 0.125), np.full(n, 0.125)
    else:
        raise ValueError(kind)
    qi_, ci_ = qi_.astype(np.float32), ci_.astype(np.float32)
    out = []
    for zero_extra in (True, False):
        qint = qi_.copy()
        qint[5] = qi_[5] if qi_[5] > 0 else qi_.max()
        extra = np.float32(0.0) if zero_extra else qint[5]
        if not zero_extra:
            qint[5] = 0.0
        q_mz = np.concatenate([qmz, [np.float32(253.0)]])
        q_in = np.concatenate([qint, [extra]]).astype(np.float32)
        order = np.argsort(q_mz, kind='stable')
        cint = ci_.copy()
        cint[5] = ci_[5] if ci_[5] > 0 else ci_.max()
        tw = np.array([7, 8, 20])
        c_mz = np.concatenate([cmz, cmz[tw] + np.float32(0.0078125)])
        c_in = np.concatenate([cint, [0.0, cint[8], cint[20]]]).astype(np.float32)
        c_ch = rng.integers(0, min(z, 3) + 1, len(c_mz)).astype(np.uint8)
        c_ch[5] = 0                     # takes part in every shift
        co = np.argsort(c_mz, kind='stable')
        out.append(((q_mz[order], q_in[order], np.zeros(n + 1, np.uint8)),
                    (c_mz[co], c_in[co], c_ch[co])))
    return out


@pytest.mark.parametrize('kind', ['denormal', 'underflow', 'zero', 'huge', 'equal'])
def test_product_range(O, kind):
    """Denormal, zero and near-overflow products and all-equal products, in the flat (z = 2), the pair
    (z = 5) and the binary-search kernel (z = 31): a zero-product match still consumes its peaks, and
    ties are resolved in generation order, so score, count AND match list equal the oracle's."""
    rng = np.random.default_rng(17)
    queries, lib, owner, l_z = [], [], [], []
    for z in (2, 5, 31):
        for rep in range(4):
            for q, c in _range_case(kind, z, rng):
                owner.append(len(queries))
                queries.append(q)
                lib.append(c)
                l_z.append(z)
    nq = len(queries)
    l_pmz = [501.5 - 3.0 / z for z in l_z]
    Qt = RC.pack(queries, [501.5] * nq, [2] * nq)
    Lt = RC.pack(lib, l_pmz, l_z)
    # the cases are what they are named for
    prod = []
    L, Q = O.Spectra(*Lt), O.Spectra(*Qt)
    for r in range(nq):
        _, s, m = O.best_match(Q, r, L, np.array([r], np.int64), 0.02, True)
        p = (Q.peaks(r)[1][m[:, 0]].astype(np.float64) * L.peaks(r)[1][m[:, 1]]).astype(np.float32)
        prod.append(p)
        assert len(m) >= 30
    prod = np.concatenate(prod)
    tiny = np.finfo(np.float32).tiny
    if kind == 'denormal':
        assert np.sum((prod > 0) & (prod < tiny)) > 100
    elif kind in ('underflow', 'zero'):
        assert np.sum(prod == 0) > 100 and np.sum(prod > 0) > 100
    elif kind == 'huge':
        assert prod.max() > 3e37 and np.all(np.isfinite(prod))
    bad = _pairs_one_to_one(O, Qt, Lt, owner, 0.02)
    assert not bad, '%d of %d pairs differ, e.g. %r' % (len(bad), nq, bad[0])
