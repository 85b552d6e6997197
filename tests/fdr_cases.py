"""Inputs shared by the CPU and GPU tests of the FDR step (ann_solo_amd/fdr.py, csrc/l2svm.hip): SVM
problems with the edge cases the kernel has to survive, and a synthetic SSM table on which the cosine
separates targets from decoys poorly and another similarity column separates them well."""
import numpy as np

from ann_solo_amd.spectral_library import SSMTable
from ann_solo_amd.spectrum_similarity import FEATURE_NAMES

#: seed of ``robust_table`` -- chosen (and checked by test_device_fdr_cpu.py) so that PercolatorTDC on the numpy
#: solver accepts more targets than the cosine, and that perturbing every fitted weight by +-1e-7 changes no label
ROBUST_SEED = 11


def svm_problems(n: int, d: int, P: int, seed: int = 0):
    """``(X [n, d], label [P, n] int8, cw [P, 2], wb0 [P, d + 1])``: P distinct problems over one matrix with
    duplicated rows. By problem index (where P allows): 0 -- generic, with rows labelled 0; 1 -- every label 0;
    2 -- a single class; 3 -- already optimal at its start (all labels 0, start 0); 4 -- linearly separable;
    5 -- a non-zero start; the rest -- random labellings, class weights from 0.1 to 10."""
    rng = np.random.default_rng([seed, n, d, P])
    X = rng.normal(size=(n, d))
    if n >= 4:
        X[n // 2] = X[0]                        # duplicated rows
        X[n - 1] = X[1]
    truth = rng.normal(size=d)
    margin = X @ truth + 0.3 * rng.normal(size=n)
    label = np.zeros((P, n), np.int8)
    cw = np.ones((P, 2))
    wb0 = np.zeros((P, d + 1))
    for p in range(P):
        noisy = np.where(margin + rng.normal(size=n) * (0.5 + 0.1 * p) > 0, 1, -1)
        label[p] = np.where(rng.random(n) < 0.2, 0, noisy)
        cw[p] = 10.0 ** rng.uniform(-1, 1, size=2)
    label[0, ::7] = 0
    if P > 1:
        label[1] = 0
    if P > 2:
        label[2] = np.where(label[2] == 0, 0, 1)
    if P > 3:
        label[3] = 0
        wb0[3] = 0.0
    if P > 4:
        label[4] = np.where(X @ truth > 0, 1, -1)       # separable (through the origin)
    if P > 5:
        wb0[5] = rng.normal(size=d + 1)
    if P > 1:
        wb0[1] = rng.normal(size=d + 1)                 # no rows: one step takes it to 0
    return X, label, cw, wb0


def synthetic_table(n_target: int, n_decoy: int, seed: int, decoys: bool = True) -> SSMTable:
    """An ``SSMTable`` of one charge-2 level with ``features``: correct targets (60 % of the targets) score
    high in ``frac_int_lib`` and only a little higher in the cosine; the other targets are distributed like
    the decoys."""
    rng = np.random.default_rng(seed)
    n = n_target + (n_decoy if decoys else 0)
    is_decoy = np.arange(n) >= n_target
    correct = (~is_decoy) & (rng.random(n) < 0.6)
    F = rng.normal(size=(n, len(FEATURE_NAMES))) * 0.05
    col = FEATURE_NAMES.index
    F[:, col('cosine')] = np.clip(0.45 + 0.1 * rng.normal(size=n) + 0.25 * correct, 0.01, 1.0)
    F[:, col('frac_int_lib')] = np.clip(0.3 + 0.1 * rng.normal(size=n) + 0.45 * correct, 0.0, 1.0)
    F[:, col('n_matched_peaks')] = rng.integers(3, 30, size=n)
    F[:, col('cosine_top5')] = F[:, col('cosine')] * 0.995 + 0.001      # correlated above 0.95: dropped
    F[:, col('kendalltau')] = 0.25                                       # constant: dropped
    F[::50, col('mse_mz')] = np.inf                                      # replaced by the finite maximum
    perm = rng.permutation(n)
    is_decoy, F = is_decoy[perm], F[perm]
    pmz = 400.0 + 600.0 * rng.random(n)
    qmeta = {2: [dict(identifier=f'scan={i}', index=i, precursor_charge=2,
                      precursor_mz=float(pmz[i] * (1 + 5e-6 * rng.normal()))) for i in range(n)]}
    lmeta = {2: [dict(identifier=i, peptide='PEPTIDEK'[:5 + i % 4] * (1 + i % 3), precursor_mz=float(pmz[i]),
                      is_decoy=bool(is_decoy[i])) for i in range(n)]}
    t = SSMTable(qmeta, lmeta)
    t.charge = np.full(n, 2, np.int32)
    t.qrow = np.arange(n, dtype=np.int64)
    t.lib_row = np.arange(n, dtype=np.int32)
    t.score = F[:, col('cosine')].copy()
    t.q = np.full(n, np.nan)
    t.batch, t.pos = np.zeros(n, np.int32), np.arange(n, dtype=np.int32)
    for name, dt, default in SSMTable._LATE:
        setattr(t, name, np.full(n, default, dt))
    t.alt_lib_row, t.alt_score = np.zeros((n, 0), np.int32), np.zeros((n, 0))
    t.delta_score, t.n_scored, t.expect = np.full(n, np.nan), np.zeros(n, np.int32), np.full(n, np.nan)
    t.features = F
    return t


def robust_table() -> SSMTable:
    return synthetic_table(3000, 3000, ROBUST_SEED)


def perturbed(solver, eps: float = 1e-7, seed: int = 5):
    """``solver`` with every fitted weight moved by a random +-eps: what another summation order may do."""
    fit, scores = solver
    rng = np.random.default_rng(seed)

    def fit_(X, label, cw, **kw):
        wb, obj, steps, status = fit(X, label, cw, **kw)
        return wb + eps * rng.choice([-1.0, 1.0], size=wb.shape), obj, steps, status
    return fit_, scores
