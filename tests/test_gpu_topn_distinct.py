"""Distinct ranked matches (asl_rescore_batch_topn_distinct / asl_search_batch_topn_distinct /
asl_rescore_knn_topn_distinct, `Config.distinct_matches`): the n best library matches of n different
groups against the oracle's best match applied n times with the winner's whole GROUP deleted
(tests/distinct_ref.py). Every comparison is exact (rows, counts and pairs equal, scores `==` as
float64) and covers every query of its batch. Beside the rule: with every group negative the bytes
of the plain top-n call, rank 0 / n_cand / knn the single-winner call's, the tiled brute-force fold
equal to the untiled one, and a repeated call the same bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

from distinct_ref import distinct_select, oracle_ranks_distinct
from test_gpu_bf_stream import UNLIMITED, _set_budget
from test_gpu_topn import (FIELDS, NS, _bytes_equal, _caller_lists, _check_query, _consistent, _postfilter,
                           _same_results, _spectra)
from test_gpu_window_scan import _queries, _tie_library, _window_mask

pytestmark = pytest.mark.gpu


def _tie_groups(n):
    """rows 0 .. 399 (the copies of one spectrum) are one group, the rest three rows a group"""
    g = (np.arange(n) // 3).astype(np.int32)
    g[:400] = 0
    return g


# ------------------------------------------------------------------ asl_rescore_batch_topn_distinct
def _raw_distinct(q, lib, cand, off, grp, tol, shift, n, stride, device):
    """asl_rescore_batch_topn_distinct with every argument in host (numpy) or device (torch) memory."""
    from ann_solo_amd import _lib
    nq = q.n
    if device:
        dev = torch.device('cuda', 0)
        q, lib = q.to(dev).contiguous(), lib.to(dev).contiguous()
        cand, off, grp = (torch.as_tensor(a, device=dev) for a in (cand, off, grp))
        mk = lambda shape, dt: torch.full(shape, -7, dtype=dt, device=dev)
        outs = (mk((nq, n), torch.int32), mk((nq, n), torch.float64), mk((nq, n), torch.int32),
                mk((nq, n, stride, 2), torch.int32))
    else:
        outs = (np.full((nq, n), -7, np.int32), np.full((nq, n), -7.0), np.full((nq, n), -7, np.int32),
                np.full((nq, n, stride, 2), 7, np.uint32))
    rc = _lib.lib().asl_rescore_batch_topn_distinct(
        _lib.peaks_struct(q), _lib.peaks_struct(lib), _lib.ptr(cand), _lib.ptr(off), _lib.ptr(grp), tol, int(shift),
        n, *[_lib.ptr(o) for o in outs], stride)
    _lib.check(rc)
    if device:
        torch.cuda.synchronize()
        outs = tuple(o.cpu().numpy() for o in outs)
        outs = outs[:3] + (outs[3].view(np.uint32),)
    return outs


@pytest.fixture(scope='module')
def seam(O):
    """64 queries x a 300-spectrum library, caller lists, four group schemes and the rule's 16 ranks of each."""
    rng = np.random.default_rng(177)
    lib = _spectra(rng, 300, [20, 50, 100, 128, 129, 200, 250], 2)
    qq = _spectra(rng, 64, [30, 127, 128, 129, 250, 60], 2)
    lists, cand, off = _caller_lists(rng, qq.n, lib.n)
    rows = np.arange(lib.n)
    by7 = (rows // 7).astype(np.int32)
    holes = by7.copy()
    holes[::3] = -1
    schemes = {'none': np.full(lib.n, -1, np.int32), 'one': np.zeros(lib.n, np.int32), 'by7': by7, 'holes': holes}
    L, Q = O.Spectra(*lib.numpy()), O.Spectra(*qq.numpy())
    tol, shift = 0.4, True
    want = {}
    for name, grp in schemes.items():
        want[name] = []
        for i in range(qq.n):
            keep = np.nonzero(lists[i] >= 0)[0]
            ranks = oracle_ranks_distinct(O, Q, i, L, lists[i][keep], grp, 16, tol, shift)
            want[name].append([(int(keep[p]), s, m) for p, _, s, m in ranks])   # position in the caller's list
    return dict(lib=lib, q=qq, lists=lists, cand=cand, off=off, schemes=schemes, want=want, tol=tol, shift=shift)


@pytest.mark.parametrize('n', NS)
def test_rescore_batch_topn_distinct_on_caller_lists(seam, n):
    from ann_solo_amd import spectrum_match
    lib, qq, lists, cand, off = (seam[k] for k in ('lib', 'q', 'lists', 'cand', 'off'))
    tol, shift, stride = seam['tol'], seam['shift'], 256
    plain = spectrum_match.rescore_batch_topn(qq, lib, cand, off, tol, shift, n, pm_stride=stride)
    one = spectrum_match.rescore_batch(qq, lib, cand, off, tol, shift, pm_stride=stride)
    skipped = twice = 0
    for name, grp in seam['schemes'].items():
        host = _raw_distinct(qq, lib, cand, off, grp, tol, shift, n, stride, device=False)
        dev = _raw_distinct(qq, lib, cand, off, grp, tol, shift, n, stride, device=True)
        wrapped = spectrum_match.rescore_batch_topn(qq, lib, cand, off, tol, shift, n, pm_stride=stride, groups=grp)
        for a, b, c in zip(host, dev, wrapped):
            assert _bytes_equal(a, b) and _bytes_equal(a, c), name
        for a, b in zip(host, one):                                   # rank 0: the plain winner
            assert _bytes_equal(a[:, 0], b), name
        for i in range(qq.n):
            _check_query(host[0][i], host[1][i], host[2][i], host[3][i], seam['want'][name][i][:n], n, (name, i))
            got = host[0][i][host[0][i] >= 0]
            g = grp[lists[i][got]]
            assert len(set(g[g >= 0])) == (g >= 0).sum(), (name, i)       # one rank per group
            r = lists[i][got]
            twice += len(set(r)) < len(r)
        if name == 'none':                                            # ungrouped: the plain call's bytes
            for a, b in zip(host, plain):
                assert _bytes_equal(a, b)
        elif name == 'one':                                           # one group: only rank 0 is filled
            assert (host[0][:, 1:] == -1).all() and not host[1][:, 1:].any() and not host[3][:, 1:].any()
        else:
            skipped += int((host[0] != plain[0]).sum())
    if n >= 5:
        assert skipped > 0          # the groups changed ranks
        assert twice > 0            # an ungrouped row listed twice took two ranks


def test_get_best_matches_with_groups(O):
    from types import SimpleNamespace
    from ann_solo_amd import spectrum_match
    rng = np.random.default_rng(5)
    lib = _spectra(rng, 12, [40, 60, 90], 2)
    qq = _spectra(rng, 1, [70], 2)
    L, Q = O.Spectra(*lib.numpy()), O.Spectra(*qq.numpy())

    def obj(p, i):
        o, mz, it, ch, pmz, pz = p.numpy()
        a, b = int(o[i]), int(o[i + 1])
        return SimpleNamespace(mz=mz[a:b], intensity=it[a:b], charge=ch[a:b], precursor_mz=float(pmz[i]),
                               precursor_charge=int(pz[i]), row=i)
    cands = [obj(lib, i) for i in range(lib.n)]
    grp = np.array([0, 0, 1, 1, -1, -1, 2, 2, 2, 3, 0, 1], np.int32)
    got = spectrum_match.get_best_matches(obj(qq, 0), cands, 0.4, True, 16, groups=grp)
    want = oracle_ranks_distinct(O, Q, 0, L, np.arange(lib.n), grp, 16, 0.4, True)
    assert len(got) == 6                                  # four groups and two ungrouped rows
    assert [c.row for c, _, _ in got] == [r for _, r, _, _ in want]
    assert [s for _, s, _ in got] == [s for _, _, s, _ in want]
    assert all(m == [tuple(x) for x in w[3].tolist()] for (_, _, m), w in zip(got, want))


# ------------------------------------------------------------------ asl_search_batch_topn_distinct, open search
def _rule_open(O, sl, q, z, tol, mode, knn, grp):
    """the rule's 16 ranks per query over (ANN id set of knn) & precursor window, ascending row"""
    part = sl.partitions[z]
    L = O.Spectra(*part.spectra.to('cpu').numpy())
    Q = O.Spectra(*q.numpy())
    key = np.ascontiguousarray(part.precursor_mz, np.float32)
    q_pmz = q.numpy()[4].astype(np.float64)
    out = []
    for i in range(q.n):
        ids = np.unique(knn[i][knn[i] >= 0])
        cand = ids[_window_mask(q_pmz[i], key[ids], z, tol, mode)].astype(np.int64)
        out.append((len(cand), [(r, s, m) for _, r, s, m in oracle_ranks_distinct(O, Q, i, L, cand, grp, 16)]))
    return out


def _check_ranks(top, want, n, what):
    for i, (n_cand, ranks) in enumerate(want):
        assert top.n_candidates[i] == n_cand, (what, i)
        _check_query(top.best_row[i], top.best_score[i], top.pm_count[i], top.pm_pairs[i], ranks[:n], n, (what, i))


@pytest.mark.parametrize('index,window', [('ivfpq', 'post'), ('ivfflat', 'post'), ('ivfpq', 'pre')])
def test_search_batch_topn_distinct_open_search(O, index, window):
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib0, aux, lib = _tie_library()
    copies = 8
    q = _queries(lib0, aux, 100, seed=73, with_copies=copies)
    grp = _tie_groups(lib.n)
    tol, mode = 250.0, 'Da'
    cfg = Config.open_search(num_list=16, num_probe=8, num_candidates=256, index=index, kmeans_niter=4,
                             precursor_tolerance_mass_open=tol, precursor_tolerance_mode_open=mode,
                             ann_window=window)
    sl = SpectralLibrary(lib, config=cfg)
    sl.set_match_groups({2: grp})
    prev = _postfilter(1)
    try:
        rules = {}
        for post in (1, 0):
            _postfilter(post)
            single = sl._search_batch(q, 2, 'open', want_knn=True)
            single_set = sl._search_batch(q, 2, 'open')
            key = single.knn.tobytes()
            if key not in rules:                      # (the same neighbours with the post-filter on and off)
                rules[key] = _rule_open(O, sl, q, 2, tol, mode, single.knn, grp)
            want = rules[key]
            for n in NS:
                what = (index, window, post, n)
                top = sl.search_batch_topn(q, 2, 'open', n, want_knn=True, distinct=True)
                _check_ranks(top, want, n, what)
                # the copy queries: the block of copies holds rank 0 and no rank below it
                assert (top.best_row[:copies, 0] < 400).all() and (top.best_row[:copies, 0] >= 0).all(), what
                assert not ((top.best_row[:copies, 1:] >= 0) & (top.best_row[:copies, 1:] < 400)).any(), what
                as_set = sl.search_batch_topn(q, 2, 'open', n, distinct=True)      # the scans' set-mode rows
                _same_results(top, as_set, what)
                _consistent(top, single, n, what=what,
                            again=sl.search_batch_topn(q, 2, 'open', n, want_knn=True, distinct=True))
                _consistent(as_set, single_set, n, what=what + ('set',))
                if n == 5:
                    plain = sl.search_batch_topn(q, 2, 'open', n, want_knn=True)
                    assert (plain.best_row[:copies] < 400).all(), what           # what the plain ranks hold
    finally:
        _postfilter(prev)
        sl.shutdown()


def test_rescore_knn_topn_distinct_equals_search_batch_topn_distinct():
    from ann_solo_amd import _lib
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    from ann_solo_amd.spectrum import HASH_SEED, get_dim
    lib0, aux, lib = _tie_library()
    q = _queries(lib0, aux, 64, seed=81, with_copies=5)
    cfg = Config.open_search(num_list=16, num_probe=8, num_candidates=256, index='ivfpq', kmeans_niter=4)
    sl = SpectralLibrary(lib, config=cfg)
    try:
        L = _lib.lib()
        h = sl.partitions[2].handle
        qd = q.to(sl.device).contiguous()
        _, min_bound, _ = get_dim(cfg.min_mz, cfg.max_mz, cfg.bin_size)
        P = _lib.AslSearchParams(min_bound, cfg.bin_size, HASH_SEED, 256, 8, 2, 300.0, 0, cfg.fragment_mz_tolerance,
                                 1, 1)
        stride = qd.max_peaks()
        idx = sl._get_ann_index(2)
        I = sl._search_batch(q, 2, 'open', want_knn=True).knn
        outs = lambda n: (np.empty((q.n, n), np.int32), np.empty((q.n, n)), np.empty(q.n, np.int32),
                          np.empty((q.n, n), np.int32), np.empty((q.n, n, stride, 2), np.uint32))

        def knn_call(n, o):
            return L.asl_rescore_knn_topn_distinct(h, C.byref(_lib.peaks_struct(qd)), C.byref(P), _lib.ptr(I), n,
                                                   *[_lib.ptr(a) for a in o], stride)

        def batch_call(n, o):
            return L.asl_search_batch_topn_distinct(h, idx._h, C.byref(_lib.peaks_struct(qd)), C.byref(P), n,
                                                    *[_lib.ptr(a) for a in o], stride, None)
        # no group column: an error of its own, never the plain ranks
        for call in (knn_call, batch_call):
            assert call(5, outs(5)) == -3
            assert b'group' in L.asl_last_error()
        with pytest.raises(_lib.AnnSoloMiError):
            sl.search_batch_topn(q, 2, 'open', 5, distinct=True)
        grp = _tie_groups(lib.n)
        assert L.asl_library_set_groups(h, lib.n - 1, _lib.ptr(grp)) == -1          # a wrong length
        assert L.asl_library_set_groups(h, lib.n + 1, _lib.ptr(grp)) == -1
        assert knn_call(5, outs(5)) == -3                                             # still no column
        for bad in (0, 17):
            assert knn_call(bad, outs(1)) == -1 and b'n_best' in L.asl_last_error()
            assert batch_call(bad, outs(1)) == -1 and b'n_best' in L.asl_last_error()
        dev_grp = torch.as_tensor(grp, device=sl.device)
        for n in NS:
            # the column from host memory and from device memory
            _lib.check(L.asl_library_set_groups(h, lib.n, _lib.ptr(grp if n % 2 else dev_grp)))
            top = sl.search_batch_topn(q, 2, 'open', n, want_knn=True, pm_stride=stride, distinct=True)
            assert np.array_equal(top.knn, I)
            o = outs(n)
            _lib.check(knn_call(n, o))
            for a, b in zip(o, (top.best_row, top.best_score, top.n_candidates, top.pm_count, top.pm_pairs)):
                assert _bytes_equal(a, b), n
        assert L.asl_library_set_groups(h, 0, None) == 0                              # dropped again
        assert knn_call(5, outs(5)) == -3 and batch_call(5, outs(5)) == -3
        plain = sl.search_batch_topn(q, 2, 'open', 5)                                 # the plain call is as it was
        sl.set_match_groups({2: np.full(lib.n, -1, np.int32)})                        # ungrouped: its bytes
        _same_results(sl.search_batch_topn(q, 2, 'open', 5, distinct=True), plain)
        with pytest.raises(ValueError):
            sl.set_match_groups({3: grp})
        sl.set_match_groups(None)
        assert knn_call(5, outs(5)) == -3
    finally:
        sl.shutdown()


# ------------------------------------------------------------------ use_ann = 0: window-only, tiled fold
def _bf(sl, q, n, budget, distinct=True):
    prev = _set_budget(budget)
    try:
        return sl.search_batch_topn(q, 2, 'open', n, distinct=distinct)
    finally:
        _set_budget(prev)


def test_window_only_distinct_fold(O):
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib0, aux, lib = _tie_library()
    copies = 8
    q = _queries(lib0, aux, 100, seed=73, with_copies=copies)
    grp = _tie_groups(lib.n)
    tol, mode = 250.0, 'Da'
    cfg = Config.open_search(mode='bf', precursor_tolerance_mass_open=tol, precursor_tolerance_mode_open=mode)
    sl = SpectralLibrary(lib, config=cfg)
    sl.set_match_groups({2: grp})
    try:
        part = sl.partitions[2]
        L = O.Spectra(*part.spectra.to('cpu').numpy())
        Q = O.Spectra(*q.numpy())
        key = np.ascontiguousarray(part.precursor_mz, np.float32)
        q_pmz = q.numpy()[4].astype(np.float64)
        order = np.argsort(key, kind='stable')                 # the library's precursor-sorted view
        runs = [order[_window_mask(q_pmz[i], key[order], 2, tol, mode)] for i in range(q.n)]
        widest = max(len(r) for r in runs)
        budget = widest // 3                                   # the widest window: at least 3 tiles
        assert budget > 16
        # the tiles cut the batch's pairs (query after query, each window in sorted order) every
        # `budget` pairs: the copies in a copy query's window lie on both sides of a cut
        pre = np.concatenate([[0], np.cumsum([len(r) for r in runs])])
        for i in range(copies):
            tiles = (pre[i] + np.nonzero(runs[i] < 400)[0]) // budget
            assert len(set(tiles.tolist())) >= 2, i
        assert max((pre[i + 1] - 1) // budget - pre[i] // budget + 1 for i in range(q.n)) >= 3
        want = []
        for i in range(q.n):
            cand = np.sort(runs[i]).astype(np.int64)
            want.append((len(cand), [(r, s, m) for _, r, s, m in oracle_ranks_distinct(O, Q, i, L, cand, grp, 16)]))
        single = _bf(sl, q, 1, UNLIMITED, distinct=False)
        for n in NS:
            full = _bf(sl, q, n, UNLIMITED)
            _check_ranks(full, want, n, ('bf', n))
            for b in (budget, 97):
                _same_results(_bf(sl, q, n, b), full, ('bf', n, b))
            assert not ((full.best_row[:copies, 1:] >= 0) & (full.best_row[:copies, 1:] < 400)).any(), n
            assert _bytes_equal(full.best_row[:, 0], single.best_row[:, 0]), n
            assert _bytes_equal(full.best_score[:, 0], single.best_score[:, 0]), n
            assert _bytes_equal(full.n_candidates, single.n_candidates), n
        sl.set_match_groups({2: np.full(lib.n, -1, np.int32)})          # ungrouped: the plain fold's bytes
        _same_results(_bf(sl, q, 5, budget), _bf(sl, q, 5, budget, distinct=False), 'ungrouped')
    finally:
        sl.shutdown()


# ------------------------------------------------------------------ the engine
def test_engine_distinct_matches():
    from ann_solo_amd import synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    base, aux = synthetic.make_library(3000, seed=95, device='cpu', charges=(2, 3), charge_p=(0.6, 0.4))
    rng = np.random.default_rng(12)
    dup = rng.choice(3000, 2000, replace=False)
    src = np.concatenate([np.arange(3000), dup])                # rows 3000 ..: replicates of rows `dup`
    lib = base.select(torch.as_tensor(src))
    peptide = lambda row: None if src[row] % 10 == 0 else 'PEP%dK' % src[row]     # every tenth: no peptide
    qs, qmeta = {}, {}
    for z in (2, 3):
        qs[z], _ = synthetic.make_queries(base, aux, 300, seed=96 + z, charge=z, open_range=250.0)
        qmeta[z] = [dict(identifier='z%d_%d' % (z, i), index=1000 * z + i, precursor_charge=z,
                         precursor_mz=float(p)) for i, p in enumerate(qs[z].precursor_mz)]
    tables, engines, n_std = {}, {}, {}
    try:
        for name, kw in (('one', dict(num_matches=1)), ('distinct', dict(num_matches=5, distinct_matches=True))):
            cfg = Config.open_search(num_list=16, num_probe=8, num_candidates=128, index='ivfpq', kmeans_niter=4,
                                     batch_size=128, **kw)
            sl = engines[name] = SpectralLibrary(lib, config=cfg)
            lmeta = {z: [dict(identifier=int(i), peptide=peptide(int(i)), precursor_mz=float(p))
                         for i, p in zip(part.ids, part.precursor_mz)] for z, part in sl.partitions.items()}

            def gate(table, mode, name=name):             # level 1 keeps the better half, the rest goes on
                table.q[:] = np.where(table.score >= np.median(table.score), 0.0, 1.0) if mode == 'std' else 0.0
                if mode == 'std':
                    n_std[name] = int((table.q < 0.01).sum())
            gate.columnar = True
            tables[name] = sl.search_packed(qs, qmeta, lmeta, score_ssms=gate)
        t1, td = tables['one'], tables['distinct']
        assert len(t1) == len(td) > 300 and 0 < n_std['one'] == n_std['distinct'] < len(td)
        for name in ('charge', 'qrow', 'lib_row', 'score', 'q'):      # identifications, scores, FDR: rank 0's
            assert _bytes_equal(getattr(t1, name), getattr(td, name)), name
        for i in range(0, len(t1), 7):
            assert np.array_equal(t1._peak_matches(i), td._peak_matches(i)), i
        assert td.alt_lib_row.shape == (len(td), 4)
        # the rule from the PLAIN ranks: a peptide has at most two spectra, so the 16 plain ranks hold
        # the five distinct ones
        sl = engines['distinct']
        pep = {z: np.array([lmeta[z][r]['peptide'] for r in range(len(lmeta[z]))], object) for z in lmeta}
        group = {}
        for z in pep:
            ids = {}
            group[z] = np.array([-1 if p is None else ids.setdefault(p, len(ids)) for p in pep[z]])
        plain16 = {(z, m): sl.search_batch_topn(qs[z], z, m, 16) for z in (2, 3) for m in ('std', 'open')}
        dist5 = {(z, m): sl.search_batch_topn(qs[z], z, m, 5, distinct=True) for z in (2, 3) for m in ('std', 'open')}
        collided = ungrouped_twice = 0
        for i in range(len(td)):
            z, r = int(td.charge[i]), int(td.qrow[i])
            m = 'std' if i < n_std['distinct'] else 'open'
            rows, scores = plain16[z, m].best_row[r], plain16[z, m].best_score[r]
            pick = distinct_select(np.where(rows >= 0, scores, -1.0), rows, group[z][np.maximum(rows, 0)], 5)
            collided += pick != list(range(len(pick)))
            want_rows = np.full(5, -1, np.int32)
            want_scores = np.zeros(5)
            want_rows[:len(pick)], want_scores[:len(pick)] = rows[pick], scores[pick]
            assert want_rows[0] == td.lib_row[i], i
            assert np.array_equal(td.alt_lib_row[i], want_rows[1:]), i
            assert np.array_equal(td.alt_score[i], want_scores[1:]), i
            assert td.delta_score[i] == want_scores[0] - want_scores[1], i
            # the alternatives are other peptides, pairwise and against the winner's
            named = [p for p in pep[z][want_rows[want_rows >= 0]] if p is not None]
            got = [pep[z][x] for x in [td.lib_row[i]] + [a for a in td.alt_lib_row[i] if a >= 0]]
            assert [p for p in got if p is not None] == named and len(set(named)) == len(named), i
            ungrouped_twice += len(got) - len(named) > 1
            for k in (1, 4):
                assert np.array_equal(td.alt_peak_matches(i, k), dist5[z, m].peak_matches(r, k)), (i, k)
            if i % 50 == 0:
                rec = td[i]
                alt = td.alt_lib_row[i]
                assert rec.delta_score == td.delta_score[i]
                assert [a[0] for a in rec.alternatives] == [int(x) for x in sl.partitions[z].ids[alt[alt >= 0]]]
        assert collided > 50 and ungrouped_twice > 0      # replicates left the ranks; ungrouped rows share them
    finally:
        for sl in engines.values():
            sl.shutdown()
