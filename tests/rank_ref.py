"""Expected ranks for the tests of asl_index_rank: the position of a target in a full neighbour row."""
import numpy as np


def neighbour_order(scores, ids):
    """ids in the index's total order: score descending, id ascending (the order of a search row)."""
    scores, ids = np.asarray(scores, np.float32), np.asarray(ids, np.int64)
    return ids[np.lexsort((ids, -scores.astype(np.float64)))]


def rank_in_row(row, target):
    """Position of ``target`` in a search row (ids in neighbour order, -1 padded), -1 when absent."""
    if target < 0:
        return -1
    hit = np.nonzero(np.asarray(row) == target)[0]
    return int(hit[0]) if len(hit) else -1


def expected_ranks(rows, targets):
    """rank_in_row per query over full-scope rows [nq, n] and one target per query."""
    return np.array([rank_in_row(rows[i], int(t)) for i, t in enumerate(targets)], np.int64)
