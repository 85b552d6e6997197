"""Inputs shared by the CPU and GPU tests of the device forest (ann_solo_amd/fdr.py ``ForestTDC``, csrc/forest.hip;
restated by tests/forest_ref.py): binned matrices with the column shapes and the label edge cases the kernels have
to survive, a float matrix for the binning, and the labelled split on which the restatement is held against
scikit-learn's forest."""
import numpy as np

#: bins per column, cycled over the columns: a constant column, two bins, one short of the maximum, the maximum,
#: then ordinary ones
BIN_COUNTS = (1, 2, 255, 256, 17, 64)
#: rows at the end of the matrix that copy row 0 (n permitting): duplicated rows, and -- as the only rows of
#: problem 3 -- rows that fall into one bin in every column
N_COPIES = 9


def binned_problems(n: int, d: int, P: int, seed: int = 0):
    """``(bins [n, 64] uint8, n_bins [d], label [P, n] int8, cw [P, 2])``. The classes follow a noisy linear
    function of the bins, so trees grow deep. By problem index (where P allows): 0 -- generic, with rows labelled
    0; 1 -- every label 0; 2 -- a single class; 3 -- only the copies of row 0, both classes: no column can split
    them; the rest -- random labellings with rows labelled 0 and class weights from 0.1 to 10 (problem 4: the
    weight of class -1 is 0)."""
    rng = np.random.default_rng([seed, n, d, P])
    n_bins = np.array([BIN_COUNTS[j % len(BIN_COUNTS)] for j in range(d)], np.int32)
    bins = np.zeros((n, 64), np.uint8)
    for j in range(d):
        bins[:, j] = rng.integers(0, n_bins[j], size=n)
    copies = np.arange(n - N_COPIES, n) if n >= 4 * N_COPIES else np.zeros(0, np.int64)
    bins[copies] = bins[0] if n else 0
    truth = rng.normal(size=d)
    margin = (bins[:, :d] / np.maximum(n_bins - 1, 1)[None, :] - 0.5) @ truth
    label = np.zeros((P, n), np.int8)
    cw = np.ones((P, 2))
    for p in range(P):
        noisy = np.where(margin + rng.normal(size=n) * (0.1 + 0.05 * p) > 0, 1, -1)
        label[p] = np.where(rng.random(n) < 0.2, 0, noisy)
        cw[p] = 10.0 ** rng.uniform(-1, 1, size=2)
    cw[0] = 1.0
    if P > 1:
        label[1] = 0
    if P > 2:
        label[2] = np.where(label[2] == 0, 0, 1)
    if P > 3:
        label[3] = 0
        label[3, copies] = np.where(np.arange(len(copies)) % 2, 1, -1)
    if P > 4:
        cw[4, 0] = 0.0
    return bins, n_bins, label, cw


def float_matrix(n: int, d: int, seed: int = 0):
    """``X [n, d]`` for the binning: by column (cycled) a constant, two distinct values, many repeated values,
    distinct values; ``-0.0`` and both infinities where n allows."""
    rng = np.random.default_rng([seed, n, d])
    X = rng.normal(size=(n, d))
    for j in range(d):
        kind = j % 4
        if kind == 0:
            X[:, j] = 7.25
        elif kind == 1:
            X[:, j] = np.where(rng.random(n) < 0.5, -1.0, 2.0)
        elif kind == 2:
            X[:, j] = np.round(X[:, j], 1)
    if n > 8 and d > 3:
        X[1, 3], X[2, 3], X[4, 2] = np.inf, -np.inf, -0.0
    return X


#: seed of the forests of ``labelled_split`` (the restatement's draws are its own: any seed will do; this is the
#: first one tried)
AUC_SEED = 1


def labelled_split():
    """The fixed split of ``fdr_cases.robust_table()``'s scaled features on which the restatement meets
    scikit-learn: ``(bins [m, 64], d, n_bins, y [m] in {+1 target, -1 decoy}, train, test)``, two thirds of the rows
    for training by a seeded permutation, binned with the training rows' edges."""
    import fdr_cases as FC
    import forest_ref as R
    from ann_solo_amd import fdr
    t = FC.robust_table()
    rows, F = fdr.feature_table(t)
    y = np.where(t.is_decoy()[rows], -1, 1).astype(np.int8)
    perm = np.random.default_rng(7).permutation(len(rows))
    train, test = np.sort(perm[:2 * len(rows) // 3]), np.sort(perm[2 * len(rows) // 3:])
    X = fdr.FeatureScaler().fit(F[train]).transform(F)
    edges, n_edges = R.bin_edges(X, train)
    return R.forest_bin(X, edges, n_edges), X.shape[1], n_edges + 1, y, train, test
