"""Reference rule of the distinct ranked matches (asl_*_topn_distinct), test side.

The ranked matches are the oracle's best match applied n times -- record the winner, delete it,
repeat (`_oracle_ranks`, tests/test_gpu_topn.py). The distinct ranks differ in the deletion alone:
after recording a winner EVERY candidate of the winner's group goes, or only the winner's slot when
its group is negative (ungrouped). `distinct_select` is the same rule on bare numbers."""
import numpy as np


def distinct_select(score, key, group, n):
    """Positions of the up to `n` distinct ranks of a list: slots walked by (score descending, key
    ascending, position ascending), a slot skipped when an earlier rank holds its (non-negative)
    group. Slots with a negative score are no candidates."""
    score, key, group = np.asarray(score, np.float64), np.asarray(key, np.int64), np.asarray(group, np.int64)
    pos = np.arange(len(score))
    order = [p for p in np.lexsort((pos, key, -score)) if score[p] >= 0.0]
    out, seen = [], set()
    for p in order:
        if len(out) == n:
            break
        g = int(group[p])
        if g >= 0 and g in seen:
            continue
        if g >= 0:
            seen.add(g)
        out.append(int(p))
    return out


def oracle_ranks_distinct(O, Q, i, L, cand, row_group, n, tol=0.02, shift=True):
    """[(position in `cand`, row, score, peak matches)]: O.best_match, the winner's group deleted
    (its slot alone when the group is negative), n times. `row_group`: group id per library row."""
    cand = np.asarray(cand, np.int64)
    row_group = np.asarray(row_group, np.int64)
    pos = np.arange(len(cand))
    out = []
    for _ in range(n):
        if len(cand) == 0:
            break
        b, s, m = O.best_match(Q, i, L, cand, tol, shift)
        assert b >= 0
        out.append((int(pos[b]), int(cand[b]), s, m))
        g = row_group[cand[b]]
        gone = (row_group[cand] == g) if g >= 0 else (np.arange(len(cand)) == b)
        cand, pos = cand[~gone], pos[~gone]
    return out
