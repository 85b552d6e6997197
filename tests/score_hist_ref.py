"""Reference side of the score histogram tests (asl_*_topn_hist, `Config.score_stats`): the histogram of
a query's candidate scores as `np.bincount` over the oracle's exact scores, an oracle-backed engine that
answers the histogram call, and the one engine case the CPU test (oracle backend) and the GPU test
(device engine) both run -- window-only (`mode='bf'`), so the two score the same candidates."""
import numpy as np
import torch

from ann_solo_amd import score_stats
from ann_solo_amd.spectral_library import Config, TopnBatchResult
from oracle_backend import OracleSpectralLibrary

BINS = 128


def pair_scores(O, Q, i, L, rows, tol=0.02, shift=True):
    """The oracle's exact scores of query i (of O.Spectra Q) against the library rows `rows`."""
    qmz, qit, _ = Q.peaks(i)
    out = np.empty(len(rows))
    for k, r in enumerate(np.asarray(rows, np.int64).tolist()):
        cmz, cit, cch = L.peaks(r)
        out[k] = O.dot_pair(qmz, qit, Q.precursor_mz[i], cmz, cit, cch, L.precursor_mz[r],
                            int(L.precursor_charge[r]), tol, shift)[0]
    return out


def hist_of(scores):
    """np.bincount of bin_of over the candidates' scores, [128] int32."""
    s = np.asarray(scores, np.float64)
    return np.bincount(score_stats.bin_of(s), minlength=BINS).astype(np.int32) if len(s) else np.zeros(BINS, np.int32)


class OracleHistLibrary(OracleSpectralLibrary):
    """OracleSpectralLibrary whose histogram call (`search_batch_topn(..., n_best=1, score_hist=True)`)
    is answered by the oracle too: the single winner of `_search_batch_local` and a numpy histogram over
    the oracle's scores of the window's rows. Window-only partitions."""

    def search_batch_topn(self, queries, charge, mode, n_best, want_knn=False, device_out=False, pm_stride=None,
                          distinct=False, windows=None, score_hist=False):
        from oracle import oracle_py as O
        assert n_best == 1 and score_hist and windows is None and not self._uses_ann(charge, mode)
        res = self._search_batch_local(queries, charge, mode)
        if res is None:
            return None
        be = self._full[charge]
        Q = O.Spectra(*queries.numpy())
        tol_val, tol_mode = be.window_tol[mode]
        hist = np.zeros((Q.n, BINS), np.int32)
        for i in range(Q.n):
            rows = np.nonzero(be._window_ok(Q.precursor_mz[i], tol_val, tol_mode))[0]
            hist[i] = hist_of(pair_scores(O, Q, i, be.L, rows, be.frag_tol, be.allow_shift))
        assert np.array_equal(hist.sum(axis=1), res.n_candidates)
        return TopnBatchResult(res.best_row[:, None], res.best_score[:, None], res.n_candidates,
                               res.pm_count[:, None], res.pm_pairs[:, None], None, hist)


def engine_case():
    """(library, queries {2: pack}, query_meta, library_meta, config kwargs): 600 spectra of charge 2, 40 queries
    half of which carry a modification of up to +-300 Da. Level 1 (20 ppm) scores a handful of candidates per
    query -- fewer than 10 losers: no expectation value --, the open level (+-300 Da over the whole library, no
    index) a few hundred."""
    from ann_solo_amd import synthetic
    lib, aux = synthetic.make_library(600, seed=31, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, 40, seed=32, charge=2, open_range=300.0)
    qmeta = {2: [dict(identifier=f'scan={i}', index=i, precursor_charge=2, precursor_mz=float(q.precursor_mz[i]))
                 for i in range(q.n)]}
    pmz = lib.precursor_mz.numpy().astype(np.float32)
    lmeta = {2: [dict(identifier=int(r), peptide=f'PEP{r}K', precursor_mz=float(p)) for r, p in enumerate(pmz)]}
    kw = dict(mode='bf', batch_size=16, precursor_tolerance_mass=20.0, precursor_tolerance_mode='ppm',
              precursor_tolerance_mass_open=300.0, precursor_tolerance_mode_open='Da')
    return lib, {2: q}, qmeta, lmeta, kw


def oracle_engine(lib, kw, **more):
    lib_np = lib.numpy()
    parts = {2: dict(lib_np=lib_np, pmz32=lib_np[4].astype(np.float32))}
    return OracleHistLibrary(parts, Config.open_search(**kw, **more), 64, 4)


del torch
