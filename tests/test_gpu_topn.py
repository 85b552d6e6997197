"""Top-n rescoring (asl_rescore_batch_topn / asl_search_batch_topn / asl_rescore_knn_topn,
`Config.num_matches`): the n best library matches per query against the oracle's best match applied
n times -- record the winner, delete it from the candidate list, repeat. On a list in ascending
library row (the reference's order) "first strict maximum wins" is "ties to the lower row"; on a
caller-ordered list it is "ties to the earlier position". Every comparison is exact (rows, counts
and pairs equal, scores `==` as float64) and covers every query of its batch. Beside the oracle:
column 0 / n_cand / knn equal the single-winner entry points bit for bit, the first two ranks of an
n = 5 call equal the n = 2 call, and a repeated call gives the same bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_bf_stream import UNLIMITED, _search, _set_budget, small          # noqa: F401 (small: a fixture)
from test_gpu_window_scan import _queries, _tie_library, _window_mask

pytestmark = pytest.mark.gpu

NS = (1, 2, 5, 16)
FIELDS = ('best_row', 'best_score', 'n_candidates', 'pm_count', 'pm_pairs')


def _oracle_ranks(O, Q, i, L, cand, n, tol=0.02, shift=True):
    """[(position in `cand`, row, score, peak matches)]: O.best_match, the winner deleted, n times."""
    cand = np.asarray(cand, np.int64)
    pos = np.arange(len(cand))
    out = []
    for _ in range(n):
        if len(cand) == 0:
            break
        b, s, m = O.best_match(Q, i, L, cand, tol, shift)
        assert b >= 0
        out.append((int(pos[b]), int(cand[b]), s, m))
        cand, pos = np.delete(cand, b), np.delete(pos, b)
    return out


def _check_query(ids, score, count, pairs, want, n, what):
    """One query's [n] outputs against the oracle's ranks (`want`: (id, score, matches) per rank)."""
    for r in range(n):
        if r >= len(want):                                   # an empty rank
            assert ids[r] == -1 and score[r] == 0.0 and count[r] == 0, (what, r)
            assert not pairs[r].any(), (what, r)
            continue
        wid, ws, wm = want[r]
        assert ids[r] == wid, (what, r, ids[:n].tolist(), [w[0] for w in want])
        assert float(score[r]) == ws, (what, r)
        assert count[r] == len(wm), (what, r)
        assert np.array_equal(pairs[r, :len(wm)], wm), (what, r)
        assert not pairs[r, len(wm):].any(), (what, r)


def _bytes_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_results(a, b, what=''):
    for f in FIELDS:
        assert _bytes_equal(getattr(a, f), getattr(b, f)), (what, f)


def _consistent(top, single, n, top2=None, top5=None, again=None, what=''):
    """column 0 = the single-winner call; the N = 5 call's first two ranks = the N = 2 call; a repeat."""
    assert _bytes_equal(top.best_row[:, 0], single.best_row), what
    assert _bytes_equal(top.best_score[:, 0], single.best_score), what
    assert _bytes_equal(top.pm_count[:, 0], single.pm_count), what
    assert _bytes_equal(top.pm_pairs[:, 0], single.pm_pairs), what
    assert _bytes_equal(top.n_candidates, single.n_candidates), what
    if single.knn is not None or top.knn is not None:
        assert _bytes_equal(top.knn, single.knn), what
    if top2 is not None:
        for f in ('best_row', 'best_score', 'pm_count', 'pm_pairs'):
            assert _bytes_equal(getattr(top5, f)[:, :2], getattr(top2, f)), (what, f)
    if again is not None:
        _same_results(top, again, what)


# ------------------------------------------------------------------ asl_rescore_batch_topn
def _spectra(rng, n, sizes, charge):
    """spectra of `sizes` peaks on a coarse m/z grid (many generated matches with a wide tolerance)."""
    from ann_solo_amd.packed import PackedSpectra
    offs, mzs, its, chs = [0], [], [], []
    for i in range(n):
        m = int(sizes[i % len(sizes)])
        g = np.sort(rng.choice(np.arange(200, 1800), size=m, replace=False)).astype(np.float32)
        mz = np.sort(g + rng.normal(0, 0.004, m).astype(np.float32))
        mzs.append(mz)
        its.append(rng.random(m).astype(np.float32) + np.float32(0.01))
        chs.append(rng.integers(0, 3, m).astype(np.uint8))
        offs.append(offs[-1] + m)
    return PackedSpectra.from_numpy(np.asarray(offs, np.int32), np.concatenate(mzs), np.concatenate(its),
                                    np.concatenate(chs), rng.uniform(400, 900, n), np.full(n, charge, np.int32))


def _caller_lists(rng, nq, n_lib):
    """caller-ordered lists: -1 entries, an empty list, lists shorter than every N > 1, rows listed twice."""
    lists = []
    for i in range(nq):
        if i == 3:
            c = np.zeros(0, np.int64)                                  # empty
        elif i == 4:
            c = np.array([-1, -1, -1], np.int64)                       # nothing valid
        elif i == 5:
            c = np.array([7], np.int64)                                # shorter than N
        elif i == 6:
            c = np.array([-1, 9, -1, 2, 9], np.int64)                  # 3 valid, a row twice
        else:
            c = rng.permutation(n_lib)[:int(rng.integers(20, 50))].astype(np.int64)
            c[rng.random(len(c)) < 0.15] = -1
            if i % 2:                                                  # a row listed twice, apart
                v = np.nonzero(c >= 0)[0]
                c[v[-1]] = c[v[0]]
        lists.append(c)
    off = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int32)
    return lists, np.concatenate(lists), off


def _raw_rescore_topn(q, lib, cand, off, tol, shift, n, stride, device):
    """asl_rescore_batch_topn with every argument in host (numpy) or device (torch) memory."""
    from ann_solo_amd import _lib
    nq = q.n
    if device:
        dev = torch.device('cuda', 0)
        q, lib = q.to(dev).contiguous(), lib.to(dev).contiguous()
        cand, off = torch.as_tensor(cand, device=dev), torch.as_tensor(off, device=dev)
        mk = lambda shape, dt: torch.full(shape, -7, dtype=dt, device=dev)
        outs = (mk((nq, n), torch.int32), mk((nq, n), torch.float64), mk((nq, n), torch.int32),
                mk((nq, n, stride, 2), torch.int32))
    else:
        outs = (np.full((nq, n), -7, np.int32), np.full((nq, n), -7.0), np.full((nq, n), -7, np.int32),
                np.full((nq, n, stride, 2), 7, np.uint32))
    rc = _lib.lib().asl_rescore_batch_topn(_lib.peaks_struct(q), _lib.peaks_struct(lib), _lib.ptr(cand),
                                           _lib.ptr(off), tol, int(shift), n, *[_lib.ptr(o) for o in outs], stride)
    _lib.check(rc)
    if device:
        torch.cuda.synchronize()
        outs = tuple(o.cpu().numpy() for o in outs)
        outs = outs[:3] + (outs[3].view(np.uint32),)
    return outs


@pytest.mark.parametrize('n', NS)
def test_rescore_batch_topn_on_caller_lists(O, n):
    from ann_solo_amd import spectrum_match
    rng = np.random.default_rng(77)
    lib = _spectra(rng, 60, [20, 50, 100, 128, 129, 200, 250], 2)     # > 128 peaks: the full-size matches launch
    qq = _spectra(rng, 24, [30, 127, 128, 129, 250, 60], 2)
    L, Q = O.Spectra(*lib.numpy()), O.Spectra(*qq.numpy())
    lists, cand, off = _caller_lists(rng, qq.n, lib.n)
    stride = 256
    big_q, big_l = np.diff(qq.numpy()[0]) > 128, np.diff(lib.numpy()[0]) > 128
    deferred = 0
    for tol, shift in ((0.02, True), (0.4, True), (0.4, False)):
        host = spectrum_match.rescore_batch_topn(qq, lib, cand, off, tol, shift, n, pm_stride=stride)
        for i in range(qq.n):
            keep = np.nonzero(lists[i] >= 0)[0]
            ranks = _oracle_ranks(O, Q, i, L, lists[i][keep], n, tol, shift)
            want = [(int(keep[p]), s, m) for p, _, s, m in ranks]      # position in the caller's list
            _check_query(host[0][i], host[1][i], host[2][i], host[3][i], want, n, (tol, shift, i))
            deferred += sum(bool(big_q[i] or big_l[row]) for _, row, _, _ in ranks)
            # a row listed twice with both copies ranked: the earlier position first
            got = [int(p) for p in host[0][i] if p >= 0]
            rows = lists[i][got]
            for a in range(len(got)):
                for b in range(a + 1, len(got)):
                    if rows[a] == rows[b]:
                        assert host[1][i][a] == host[1][i][b] and got[a] < got[b]
        one = spectrum_match.rescore_batch(qq, lib, cand, off, tol, shift, pm_stride=stride)
        for a, b in zip(host, one):
            assert _bytes_equal(a[:, 0], b), (tol, shift)
        dev = _raw_rescore_topn(qq, lib, cand, off, tol, shift, n, stride, device=True)
        raw = _raw_rescore_topn(qq, lib, cand, off, tol, shift, n, stride, device=False)
        for a, b, c in zip(host, dev, raw):
            assert _bytes_equal(a, b) and _bytes_equal(a, c), (tol, shift)
        if n == 5:
            two = spectrum_match.rescore_batch_topn(qq, lib, cand, off, tol, shift, 2, pm_stride=stride)
            for a, b in zip(host, two):
                assert _bytes_equal(a[:, :2], b), (tol, shift)
    assert deferred > n              # winners beyond the small matches kernel's 128 peaks were emitted


def test_get_best_matches_dropin(O):
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
    got = spectrum_match.get_best_matches(obj(qq, 0), cands, 0.4, True, 5)
    want = _oracle_ranks(O, Q, 0, L, np.arange(lib.n), 5, 0.4, True)
    assert [c.row for c, _, _ in got] == [r for _, r, _, _ in want]
    assert [s for _, s, _ in got] == [s for _, _, s, _ in want]
    assert all(m == [tuple(x) for x in w[3].tolist()] for (_, _, m), w in zip(got, want))
    one = spectrum_match.get_best_match(obj(qq, 0), cands, 0.4, True)
    assert one[0].row == got[0][0].row and one[1] == got[0][1] and one[2] == got[0][2]
    assert len(spectrum_match.get_best_matches(obj(qq, 0), cands[:3], 0.4, True, 16)) == 3


# ------------------------------------------------------------------ asl_search_batch_topn, open search
def _postfilter(on):
    from ann_solo_amd import _lib
    return _lib.lib().asl_set_scan_postfilter(int(on))


def _check_open(O, sl, q, z, tol, mode, top, n, what):
    """expected = the oracle's ranks over (ANN id set of knn) & precursor window & validity, ascending row"""
    part = sl.partitions[z]
    L = O.Spectra(*part.spectra.to('cpu').numpy())
    Q = O.Spectra(*q.numpy())
    key = np.ascontiguousarray(part.precursor_mz, np.float32)
    q_pmz = q.numpy()[4].astype(np.float64)
    spans = 0
    for i in range(q.n):
        ids = np.unique(top.knn[i][top.knn[i] >= 0])
        cand = ids[_window_mask(q_pmz[i], key[ids], z, tol, mode)].astype(np.int64)
        assert top.n_candidates[i] == len(cand), (what, i)
        ranks = _oracle_ranks(O, Q, i, L, cand, n)
        _check_query(top.best_row[i], top.best_score[i], top.pm_count[i], top.pm_pairs[i],
                     [(r, s, m) for _, r, s, m in ranks], n, (what, i))
        sc = [s for _, _, s, _ in ranks]
        spans += len(sc) > 2 and sc[0] == sc[1] == sc[2]
    return spans


@pytest.mark.parametrize('index,window', [('ivfpq', 'post'), ('ivfflat', 'post'), ('ivfpq', 'pre')])
def test_search_batch_topn_open_search(O, index, window):
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib0, aux, lib = _tie_library()
    q = _queries(lib0, aux, 64, seed=73, with_copies=6)
    tol, mode = 250.0, 'Da'
    cfg = Config.open_search(num_list=16, num_probe=8, num_candidates=256, index=index, kmeans_niter=4,
                             precursor_tolerance_mass_open=tol, precursor_tolerance_mode_open=mode,
                             ann_window=window)
    sl = SpectralLibrary(lib, config=cfg)
    prev = _postfilter(1)
    try:
        for post in (1, 0):
            _postfilter(post)
            single = sl._search_batch(q, 2, 'open', want_knn=True)
            single_set = sl._search_batch(q, 2, 'open')
            tops = {}
            for n in NS:
                top = tops[n] = sl.search_batch_topn(q, 2, 'open', n, want_knn=True)
                spans = _check_open(O, sl, q, 2, tol, mode, top, n, (index, window, post, n))
                if n >= 5:
                    assert spans > 0             # equal scores span several ranks (the copies of row 0)
                as_set = sl.search_batch_topn(q, 2, 'open', n)       # the scans' set-mode rows
                _same_results(top, as_set, (index, window, post, n))
                _consistent(top, single, n, again=sl.search_batch_topn(q, 2, 'open', n, want_knn=True),
                            what=(index, window, post, n))
                _consistent(as_set, single_set, n, what=(index, window, post, n, 'set'))
            _consistent(tops[5], single, 5, tops[2], tops[5])
            dev = sl.search_batch_topn(q.to('cuda:0'), 2, 'open', 5, want_knn=True, device_out=True)
            torch.cuda.synchronize()
            for f in FIELDS:
                got = getattr(dev, f).cpu().numpy()
                assert _bytes_equal(got.view(getattr(tops[5], f).dtype), getattr(tops[5], f)), f
    finally:
        _postfilter(prev)
        sl.shutdown()


def test_rescore_knn_topn_equals_search_batch_topn():
    from ann_solo_amd import _lib
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    from ann_solo_amd.spectrum import HASH_SEED, get_dim
    lib0, aux, lib = _tie_library()
    q = _queries(lib0, aux, 64, seed=81, with_copies=5)
    cfg = Config.open_search(num_list=16, num_probe=8, num_candidates=256, index='ivfpq', kmeans_niter=4)
    sl = SpectralLibrary(lib, config=cfg)
    try:
        idx = sl._get_ann_index(2)
        qd = q.to(sl.device).contiguous()
        _, I = idx.search(sl._encode(qd), 256)                     # asl_index_search
        I = np.ascontiguousarray(torch.as_tensor(I).cpu().numpy(), np.int64)
        _, min_bound, _ = get_dim(cfg.min_mz, cfg.max_mz, cfg.bin_size)
        P = _lib.AslSearchParams(min_bound, cfg.bin_size, HASH_SEED, 256, 8, 2, 300.0, 0, cfg.fragment_mz_tolerance,
                                 1, 1)
        stride = qd.max_peaks()
        for n in NS:
            top = sl.search_batch_topn(q, 2, 'open', n, want_knn=True, pm_stride=stride)
            assert np.array_equal(top.knn, I)
            row, sc = np.empty((q.n, n), np.int32), np.empty((q.n, n))
            nc, cnt = np.empty(q.n, np.int32), np.empty((q.n, n), np.int32)
            pairs = np.empty((q.n, n, stride, 2), np.uint32)
            _lib.check(_lib.lib().asl_rescore_knn_topn(
                sl.partitions[2].handle, C.byref(_lib.peaks_struct(qd)), C.byref(P), _lib.ptr(I), n,
                _lib.ptr(row), _lib.ptr(sc), _lib.ptr(nc), _lib.ptr(cnt), _lib.ptr(pairs), stride))
            for a, b in ((row, top.best_row), (sc, top.best_score), (nc, top.n_candidates), (cnt, top.pm_count),
                         (pairs, top.pm_pairs)):
                assert _bytes_equal(a, b), n
        L = _lib.lib()
        for bad in (0, 17):
            assert L.asl_rescore_knn_topn(sl.partitions[2].handle, C.byref(_lib.peaks_struct(qd)), C.byref(P),
                                          _lib.ptr(I), bad, None, None, None, None, None, stride) == -1
            assert b'n_best' in L.asl_last_error()
    finally:
        sl.shutdown()


# ------------------------------------------------------------------ use_ann = 0: window-only, tiled
def _topn_budget(sl, q, mode, n, budget):
    prev = _set_budget(budget)
    try:
        return sl.search_batch_topn(q, 2, mode, n)
    finally:
        _set_budget(prev)


@pytest.mark.parametrize('mode,tol,tmode', [('open', 300, 'Da'), ('std', 20, 'ppm')])
def test_window_only_topn_tiles_and_oracle(O, small, mode, tol, tmode):
    sl, lib, valid, q, special, dup = small
    part = sl.partitions[2]
    L = O.Spectra(*part.spectra.to('cpu').numpy())
    Q = O.Spectra(*q.numpy())
    pmz32 = part.precursor_mz
    cands = []
    for i in range(q.n):
        near = np.nonzero(np.abs(pmz32.astype(np.float64) - Q.precursor_mz[i]) <= 200.0)[0]
        cands.append(np.array([r for r in near if valid[r] and
                               O.precursor_ok(Q.precursor_mz[i], pmz32[r], 2, tol, tmode)], np.int64))
    assert len(cands[88]) == 0                                     # the empty window
    assert any(0 < len(c) < 5 for c in cands) or mode == 'open'    # windows of fewer than N rows (20 ppm)
    ranks16 = [_oracle_ranks(O, Q, i, L, cands[i], 16) for i in range(q.n)]
    prev = _set_budget(UNLIMITED)
    try:
        single = sl._search_batch(q, 2, mode)
    finally:
        _set_budget(prev)
    fulls = {}
    for n in NS:
        full = fulls[n] = _topn_budget(sl, q, mode, n, UNLIMITED)
        for budget in (1, 7, 1000):                 # 1: every pair a tile of its own
            tiled = _topn_budget(sl, q, mode, n, budget)
            _same_results(tiled, full, (mode, n, budget))
            if n == 1 and budget < 1000:
                # the single-winner search at the same cuts: one fold and one matches kernel serve both,
                # only the selection differs (argmax / ranked), so every output is the same
                _consistent(tiled, _search(sl, q, mode, budget), 1, what=(mode, 'single', budget))
        sub = _topn_budget(sl, q.select(torch.as_tensor(special)), mode, n, 1)
        for f in FIELDS:
            assert _bytes_equal(getattr(sub, f), getattr(full, f)[special]), (mode, n, f)
        for i in range(q.n):
            assert full.n_candidates[i] == len(cands[i]), i
            _check_query(full.best_row[i], full.best_score[i], full.pm_count[i], full.pm_pairs[i],
                         [(r, s, m) for _, r, s, m in ranks16[i][:n]], n, (mode, n, i))
        _consistent(full, single, n, again=_topn_budget(sl, q, mode, n, 1000), what=(mode, n))
    _consistent(fulls[5], single, 5, fulls[2], fulls[5])
    if mode == 'open':
        # n = ASL_MAX_BEST at budget 1 above filled the fold's result to its last entry, without groups
        assert (fulls[16].best_row[:, 15] >= 0).any()
        # a library spectrum as query: the original and its copy tie, the lower row first
        tied = sum(fulls[2].best_score[i, 0] == fulls[2].best_score[i, 1] and
                   fulls[2].best_row[i, 0] < fulls[2].best_row[i, 1] for i in range(68, 88))
        assert tied > 10


# ------------------------------------------------------------------ errors, pipeline
def test_bad_rank_counts_and_pipelined_batches_in_flight():
    from ann_solo_amd import _lib, synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    from ann_solo_amd.spectrum import HASH_SEED, get_dim
    lib, aux = synthetic.make_library(6000, seed=91, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, 512, seed=92, charge=2)
    cfg = Config.open_search(num_list=32, num_probe=8, num_candidates=128, index='ivfpq', kmeans_niter=4)
    sl = SpectralLibrary(lib, config=cfg)
    try:
        L = _lib.lib()
        idx = sl._get_ann_index(2)
        qd = q.to('cuda:0').contiguous()
        _, min_bound, _ = get_dim(cfg.min_mz, cfg.max_mz, cfg.bin_size)
        P = _lib.AslSearchParams(min_bound, cfg.bin_size, HASH_SEED, 128, 8, 2, 300.0, 0, 0.02, 1, 1)
        for bad in (0, 17, -1):
            assert L.asl_search_batch_topn(sl.partitions[2].handle, idx._h, C.byref(_lib.peaks_struct(qd)),
                                           C.byref(P), bad, None, None, None, None, None, 0, None) == -1
            assert b'n_best' in L.asl_last_error()
            with pytest.raises(_lib.AnnSoloMiError):
                sl.search_batch_topn(q, 2, 'open', bad)
        cand = np.zeros(1, np.int64)
        off = np.array([0, 1], np.int32)
        one = q.select(torch.arange(1))
        for bad in (0, 17):
            assert L.asl_rescore_batch_topn(_lib.peaks_struct(one), _lib.peaks_struct(lib), _lib.ptr(cand),
                                            _lib.ptr(off), 0.02, 1, bad, None, None, None, None, 0) == -1
            assert b'n_best' in L.asl_last_error()
        sync = sl._search_batch(qd, 2, 'open', device_out=True)
        want = sl.search_batch_topn(q, 2, 'open', 5)
        sl.set_pipeline(True)
        try:
            a = sl._search_batch(qd, 2, 'open', device_out=True)
            b = sl._search_batch(qd, 2, 'open', device_out=True)
            top = sl.search_batch_topn(q, 2, 'open', 5)            # waits for a and b, then runs
            c = sl._search_batch(qd, 2, 'open', device_out=True)   # joins the pipeline again
            sl.synchronize()
        finally:
            sl.set_pipeline(False)
        _same_results(top, want)
        for r in (a, b, c):
            for f in FIELDS:
                assert torch.equal(getattr(r, f), getattr(sync, f)), f
        assert _bytes_equal(want.best_row[:, 0], sync.best_row.cpu().numpy())
    finally:
        sl.shutdown()


# ------------------------------------------------------------------ the engine
def test_engine_num_matches(O):
    from ann_solo_amd import synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, aux = synthetic.make_library(5000, seed=95, device='cpu', charges=(2, 3), charge_p=(0.6, 0.4))
    qs, qmeta = {}, {}
    for z in (2, 3):
        qs[z], _ = synthetic.make_queries(lib, aux, 300, seed=96 + z, charge=z, open_range=250.0)
        qmeta[z] = [dict(identifier='z%d_%d' % (z, i), index=1000 * z + i, precursor_charge=z,
                         precursor_mz=float(p)) for i, p in enumerate(qs[z].precursor_mz)]
    tables, engines, n_std = {}, {}, {}
    try:
        for n in (1, 3):
            cfg = Config.open_search(num_list=16, num_probe=8, num_candidates=128, index='ivfpq', kmeans_niter=4,
                                     batch_size=128, num_matches=n)
            sl = engines[n] = SpectralLibrary(lib, config=cfg)
            lmeta = {z: [dict(identifier=int(i), peptide='PEP%dK' % i, precursor_mz=float(p))
                         for i, p in zip(part.ids, part.precursor_mz)] for z, part in sl.partitions.items()}

            def gate(table, mode, n=n):                  # level 1 keeps the better half, the rest goes on
                table.q[:] = np.where(table.score >= np.median(table.score), 0.0, 1.0) if mode == 'std' else 0.0
                if mode == 'std':
                    n_std[n] = int((table.q < 0.01).sum())
            gate.columnar = True
            tables[n] = sl.search_packed(qs, qmeta, lmeta, score_ssms=gate)
        t1, t3 = tables[1], tables[3]
        assert len(t1) == len(t3) > 300 and 0 < n_std[1] == n_std[3] < len(t3)
        for name in ('charge', 'qrow', 'lib_row', 'score', 'q'):
            assert _bytes_equal(getattr(t1, name), getattr(t3, name)), name
        for i in range(len(t1)):
            assert np.array_equal(t1._peak_matches(i), t3._peak_matches(i)), i
        assert t1.alt_lib_row.shape == (len(t1), 0) and np.isnan(t1.delta_score).all()
        assert t3.alt_lib_row.shape == (len(t3), 2) and (t3.alt_lib_row >= 0).any()
        # the alt_* columns are the batch-level call's ranks 1.., the gap is rank 0 minus rank 1; the
        # identifications of level 1 come first in the table
        sl = engines[3]
        tops = {(z, mode): sl.search_batch_topn(qs[z], z, mode, 3) for z in (2, 3) for mode in ('std', 'open')}
        lone = 0
        for i in range(len(t3)):
            z, r = int(t3.charge[i]), int(t3.qrow[i])
            top = tops[z, 'std' if i < n_std[3] else 'open']
            assert top.best_row[r, 0] == t3.lib_row[i], i
            assert np.array_equal(t3.alt_lib_row[i], top.best_row[r, 1:]), i
            assert np.array_equal(t3.alt_score[i], top.best_score[r, 1:]), i
            assert t3.delta_score[i] == top.best_score[r, 0] - top.best_score[r, 1], i
            if top.best_row[r, 1] < 0:
                lone += 1
                assert t3.delta_score[i] == top.best_score[r, 0], i
            for k in (1, 2):
                assert np.array_equal(t3.alt_peak_matches(i, k), top.peak_matches(r, k)), (i, k)
            rec = t3[i]
            assert rec.delta_score == t3.delta_score[i] and rec.library_identifier == sl.partitions[z].ids[t3.lib_row[i]]
            alt = top.best_row[r, 1:]
            assert [a[0] for a in rec.alternatives] == [int(x) for x in sl.partitions[z].ids[alt[alt >= 0]]]
            assert [a[1] for a in rec.alternatives] == [float(x) for x in top.best_score[r, 1:][alt >= 0]]
        assert lone > 0               # 20 ppm windows with a single candidate: the gap is the score itself
    finally:
        for sl in engines.values():
            sl.shutdown()
