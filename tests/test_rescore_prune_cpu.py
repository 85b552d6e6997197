"""The premise of the pruning of deferred candidates (csrc/rescore.hip: rescore_flat_kernel), on the
CPU: the sum of ALL generated matches of a pair bounds its score from above, the pairs with a
repeated peak are the ones the greedy pass has to resolve, and tests/prune_cases.py plants what
tests/test_gpu_rescore_prune.py counts on -- with margins so wide that the kernels' counters are
exactly predictable. Without this the GPU test could pass on cases in which nothing is pruned."""
import numpy as np
import pytest

import prune_cases as PC
import rescore_cases as RC


def _check_pair(O, qmz, qit, qpmz, cmz, cit, cch, cpmz, cz, tol):
    """One pair: the ported generation loop against the oracle. Returns (deferred, bound, score)."""
    m = PC.match_list(qmz, qit, qpmz, cmz, cit, cch, cpmz, cz, tol, True)
    s, greedy = O.dot_pair(qmz, qit, qpmz, cmz, cit, cch, cpmz, cz, tol, True)
    bound, repeats, signed = PC.bound_of(m)
    # the greedy pass accepts a subset of the generated matches ...
    gen = {(q, c) for _, q, c in m}
    assert all((int(q), int(c)) in gen for q, c in greedy)
    assert len(greedy) <= len(m)
    # ... all of them exactly when no peak repeats: those are the pairs that need the pass
    assert (len(greedy) == len(m)) == (not repeats)
    if not signed:
        # products >= 0: the score sums a subset of what the bound sums (fp64 rounding of the two
        # sums: a few hundred terms of relative error 2^-53 each)
        assert s <= bound * (1.0 + 1e-12) + 1e-300
        if not repeats:
            # and the same numbers when nothing repeats: equal up to the order of the additions
            assert abs(s - bound) <= 1e-12 * bound
    return repeats or signed, bound, s


@pytest.mark.parametrize('number', [1, 4, 5])
def test_bound_holds_on_the_numeric_regimes(O, number):
    """Every planted pair of tests/rescore_cases.py regimes 1, 4 and 5 (window edges, large m/z,
    far precursors, precursor charges up to 30)."""
    n = n_def = 0
    for block in RC.regime_blocks(number):
        qo, qmz, qit, _, qpmz, _ = block.queries
        lo, lmz, lit, lch, lpmz, lz = block.library
        for r in range(block.nlib):
            q = int(block.owner[r])
            a, b = slice(qo[q], qo[q + 1]), slice(lo[r], lo[r + 1])
            d, _, _ = _check_pair(O, qmz[a], qit[a], qpmz[q], lmz[b], lit[b], lch[b], lpmz[r], int(lz[r]),
                                  block.tol)
            n, n_def = n + 1, n_def + bool(d)
    print('regime %d: %d pairs, %d with a repeated peak' % (number, n, n_def))
    assert n_def > 0 and n_def < n


@pytest.mark.parametrize('name', sorted(PC.CASES))
def test_bound_holds_on_the_planted_cases(O, name):
    case = PC.get(name)
    qo, qmz, qit, _, qpmz, _ = case.queries
    lo, lmz, lit, lch, lpmz, lz = case.library
    for qi, rows in enumerate(case.lists):
        for r in rows:
            a, b = slice(qo[qi], qo[qi + 1]), slice(lo[r], lo[r + 1])
            _check_pair(O, qmz[a], qit[a], qpmz[qi], lmz[b], lit[b], lch[b], lpmz[r], int(lz[r]), PC.TOL)


def _margins(rec, best):
    """Every deferred candidate with a bound is far on one side of the best exact score."""
    for r, bound, s, deferred, pruned in rec:
        if deferred and best > 0.0 and np.isfinite(bound) and bound >= 0.0:
            assert bound <= 0.5 * best or bound >= best + 1e-3, (r, bound, best)


def test_case_a_deferred_winner(O):
    case = PC.get('a')
    for qi, (n_def, n_pruned, rec, best) in enumerate(PC.expected_counts(O, case)):
        _margins(rec, best)
        by_row = {r: x for r, *x in rec}
        w = int(case.lists[qi].min()) + case.notes['winner_local']
        bound, s, deferred, pruned = by_row[w]
        assert deferred and not pruned and bound == max(x[0] for x in by_row.values())
        assert s == max(x[1] for x in by_row.values()) and s > best        # it wins, over the best exact score
        assert n_pruned == n_def - 1 and n_pruned >= 5


def test_case_b_bound_above_score_below(O):
    case = PC.get('b')
    for qi, (n_def, n_pruned, rec, best) in enumerate(PC.expected_counts(O, case)):
        _margins(rec, best)
        by_row = {r: x for r, *x in rec}
        base = int(case.lists[qi].min())
        bound, s, deferred, pruned = by_row[base + case.notes['loser_local']]
        assert deferred and not pruned and s < best < bound
        assert by_row[base + case.notes['winner_local']][1] == best
        assert n_pruned == n_def - 1 and n_pruned >= 5


def test_case_c_tie(O):
    case = PC.get('c')
    Q, L = O.Spectra(*case.queries), O.Spectra(*case.library)
    for qi, (n_def, n_pruned, rec, best) in enumerate(PC.expected_counts(O, case)):
        _margins(rec, best)
        by_row = {r: x for r, *x in rec}
        base = int(case.lists[qi].min())
        x, y = base + case.notes['x_local'], base + case.notes['y_local']
        assert by_row[x][1] == by_row[y][1] == best                       # the same bits
        assert not by_row[x][2] and by_row[y][2] and not by_row[y][3]     # Y deferred, not pruned
        assert by_row[y][0] >= best + 1e-3
        rows = case.lists[qi]
        b, _, _ = O.best_match(Q, qi, L, rows, PC.TOL, True)              # first position: X
        assert rows[b] == x
        b, _, _ = O.best_match(Q, qi, L, np.sort(rows), PC.TOL, True)     # ascending rows: Y
        assert np.sort(rows)[b] == y
        assert n_pruned == n_def - 1 and n_pruned >= 5


def test_case_d_everything_deferred(O):
    case = PC.get('d')
    for n_def, n_pruned, rec, best in PC.expected_counts(O, case):
        assert n_def == PC.N_CAND and n_pruned == 0 and best == 0.0


def test_case_e_best_in_the_second_super_chunk(O):
    case = PC.get('e')
    (n_def, n_pruned, rec, best), = PC.expected_counts(O, case)
    _margins(rec, best)
    assert len(rec) == 1030 and rec[case.notes['winner_local']][2] == best
    slots = [i for i, x in enumerate(rec) if x[3]]
    assert len(slots) >= 20 and max(slots) < 1024 <= case.notes['winner_local']
    assert n_pruned == n_def
    first = max(x[2] for x in rec[:1024] if not x[3])
    assert all(rec[i][1] > first + 1e-3 for i in slots)      # not prunable inside the first super-chunk


def test_case_f_negative_intensity(O):
    case = PC.get('f')
    assert (case.queries[2] < 0).sum() == case.nq
    for n_def, n_pruned, rec, best in PC.expected_counts(O, case):
        assert n_def >= 8 and n_pruned == 0
        assert all(s > 0 for _, _, s, _, _ in rec)           # (a negative total is not a valid score)
        assert best == max(s for _, _, s, _, _ in rec)
