"""The argument contract of the six batch entry points -- asl_search_batch, asl_search_batch_topn,
asl_search_batch_topn_distinct, asl_rescore_knn, asl_rescore_knn_topn, asl_rescore_knn_topn_distinct -- as one
table: which bad argument gives which return code, which check goes first where the codes differ, that an
empty batch is ASL_OK and writes nothing, and that a rejected call leaves nothing behind: the outputs keep
their sentinels and the next valid call on the same handles returns the bytes it returned before.

Every case is rejected by the host-side checks before anything is launched; no case hands a kernel bad data
(no out-of-range rows, no undersized buffers). 64 synthetic spectra of one charge, 4 queries, an IVF-Flat
index of 4 lists, k = 8, n_best = 2, groups of two rows."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, INVALID, STATE = 0, -1, -3
K, N_BEST, NQ = 8, 2, 4
ENTRIES = ['asl_search_batch', 'asl_search_batch_topn', 'asl_search_batch_topn_distinct',
           'asl_rescore_knn', 'asl_rescore_knn_topn', 'asl_rescore_knn_topn_distinct']
topn = lambda e: 'topn' in e
distinct = lambda e: 'distinct' in e
knn = lambda e: 'knn' in e
every = lambda e: True

# (what, the entries it applies to, the arguments it changes, the code, a word of the message or None)
# arguments: h, idx, q (None: null; 0: an empty batch), P (None: null; a dict: fields changed), I, n, pairs
# (False: no pm_pairs), stride, groups (False: the library's group column dropped for the call)
CASES = [
    ('n_best 0', topn, dict(n=0), INVALID, b'n_best'),
    ('n_best 17', topn, dict(n=17), INVALID, b'n_best'),
    ('n_best -1', topn, dict(n=-1), INVALID, b'n_best'),
    ('n_best goes before the nulls', topn, dict(n=0, h=None, q=None, P=None), INVALID, b'n_best'),
    ('null library', every, dict(h=None), INVALID, None),
    ('null queries', every, dict(q=None), INVALID, None),
    ('null params', every, dict(P=None), INVALID, None),
    ('null neighbour list', knn, dict(I=None), INVALID, None),
    ('no group column', distinct, dict(groups=False), STATE, b'group'),
    ('no group column, decided before the empty batch', distinct, dict(groups=False, q=0), STATE, b'group'),
    ('no group column goes before pm_stride', distinct, dict(groups=False, stride=0), STATE, b'group'),
    ('empty batch', every, dict(q=0), OK, None),
    ('empty batch goes before pm_stride', every, dict(q=0, stride=0), OK, None),
    ('pm_pairs with pm_stride 0', every, dict(stride=0), INVALID, b'pm_stride'),
    ('pm_pairs with pm_stride -1', every, dict(stride=-1), INVALID, b'pm_stride'),
    ('use_ann without an index', lambda e: not knn(e), dict(idx=None), INVALID, b'index'),
    ('k 0', every, dict(P=dict(k=0)), INVALID, b'k must'),
    ('k -8', every, dict(P=dict(k=-8)), INVALID, b'k must'),
    ('interval mode without precursor_window', every, dict(P=dict(precursor_mode=2)), INVALID, b'precursor_window'),
    ('score flag word 4', every, dict(P=dict(allow_shift=4)), INVALID, b'allow_shift'),
    ('score flag word 1 | 8', every, dict(P=dict(allow_shift=9)), INVALID, b'allow_shift'),
]
# pm_stride is not read without pm_pairs: a valid call, the same winners
VALID_VARIANTS = [('no pm_pairs, pm_stride 0', dict(pairs=False, stride=0))]


@pytest.fixture(scope='module')
def world():
    import torch
    from ann_solo_amd import _lib, synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    from ann_solo_amd.spectrum import HASH_SEED, get_dim
    lib, aux = synthetic.make_library(64, seed=11, device='cpu', charges=(2,), charge_p=(1.0,))
    q, _ = synthetic.make_queries(lib, aux, NQ, seed=12, charge=2)
    cfg = Config.open_search(num_list=4, num_probe=2, num_candidates=K, index='ivfflat', kmeans_niter=4)
    sl = SpectralLibrary(lib, config=cfg)
    L = _lib.lib()
    qd = q.to(sl.device).contiguous()
    _, min_bound, _ = get_dim(cfg.min_mz, cfg.max_mz, cfg.bin_size)
    w = dict(L=L, lib=_lib, sl=sl, h=sl.partitions[2].handle, idx=sl._get_ann_index(2)._h, qd=qd,
             stride=qd.max_peaks(), grp=(np.arange(lib.n) // 2).astype(np.int32), torch=torch,
             P=dict(min_bound=min_bound, bin_size=cfg.bin_size, hash_seed=HASH_SEED, k=K, nprobe=2, charge=2,
                    precursor_tol=300.0, precursor_mode=0, fragment_mz_tolerance=cfg.fragment_mz_tolerance,
                    allow_shift=1, use_ann=1))
    _lib.check(L.asl_library_set_groups(w['h'], lib.n, _lib.ptr(w['grp'])))
    # the neighbour lists the asl_rescore_knn* calls are given: the index's own, every id a library row or -1
    I = np.full((NQ, K), -7, np.int64)
    o = _outs(w, 1)
    _lib.check(L.asl_search_batch(w['h'], w['idx'], C.byref(_lib.peaks_struct(qd)), C.byref(_params(w, {})),
                                  *[_lib.ptr(a) for a in o], w['stride'], _lib.ptr(I)))
    assert ((I >= -1) & (I < lib.n)).all() and (I >= 0).any()
    w['I'] = I
    yield w
    sl.shutdown()


def _params(w, changed):
    return w['lib'].AslSearchParams(**{**w['P'], **changed})


def _outs(w, n):
    """best_row, best_score, n_cand, pm_count, pm_pairs: sentinel-filled host arrays"""
    return (np.full((NQ, n), -7, np.int32), np.full((NQ, n), -7.0), np.full(NQ, -7, np.int32),
            np.full((NQ, n), -7, np.int32), np.full((NQ, n, w['stride'], 2), 7, np.uint32))


def _call(w, entry, o, h='h', idx='idx', q='q', P=(), I='I', n=N_BEST, pairs=True, stride=None, groups=True):
    """One call of `entry`; the keyword arguments replace the valid ones (see CASES). Returns the code and the
    message the call left."""
    lib, L = w['lib'], w['L']
    if groups is False:
        assert L.asl_library_set_groups(w['h'], 0, None) == OK
    try:
        qs = lib.peaks_struct(w['qd'])          # (holds raw pointers into w['qd'])
        if q == 0:
            qs.n = 0
        args = [w['h'] if h == 'h' else h]
        if not knn(entry):
            args.append(w['idx'] if idx == 'idx' else idx)
        args += [None if q is None else C.byref(qs), None if P is None else C.byref(_params(w, dict(P)))]
        if knn(entry):
            args.append(lib.ptr(w['I']) if isinstance(I, str) else I)
        if topn(entry):
            args.append(n)
        args += [lib.ptr(a) for a in o[:4]] + [lib.ptr(o[4]) if pairs else None,
                                               w['stride'] if stride is None else stride]
        if not knn(entry):
            args.append(None)                   # no ordered neighbour list back
        return getattr(L, entry)(*args), L.asl_last_error() or b''
    finally:
        if groups is False:
            lib.check(L.asl_library_set_groups(w['h'], len(w['grp']), lib.ptr(w['grp'])))


def _untouched(w, o, n):
    return all(a.tobytes() == b.tobytes() for a, b in zip(o, _outs(w, n)))


@pytest.mark.parametrize('entry', ENTRIES)
def test_argument_contract(world, entry):
    w = world
    n = N_BEST if topn(entry) else 1
    before = _outs(w, n)
    assert _call(w, entry, before)[0] == OK, w['L'].asl_last_error()
    assert (before[0] >= 0).any() and (before[2] > 0).any()          # the valid call finds matches
    ran = 0
    for what, applies, changed, code, word in CASES:
        if not applies(entry):
            continue
        ran += 1
        o = _outs(w, n)
        rc, msg = _call(w, entry, o, **changed)
        print(entry, what, rc, msg)
        assert rc == code, (entry, what, rc, msg)
        assert (msg == b'') == (code == OK), (entry, what, msg)
        if word is not None:
            assert word in msg, (entry, what, msg)
        assert _untouched(w, o, n), (entry, what)                     # rejected or empty: nothing written
        after = _outs(w, n)                                           # and nothing left behind
        assert _call(w, entry, after)[0] == OK, (entry, what, w['L'].asl_last_error())
        assert all(a.tobytes() == b.tobytes() for a, b in zip(after, before)), (entry, what)
    assert ran == 13 + 4 * topn(entry) + 3 * distinct(entry)          # every case that applies was reached
    for what, changed in VALID_VARIANTS:
        o = _outs(w, n)
        assert _call(w, entry, o, **changed)[0] == OK, (entry, what, w['L'].asl_last_error())
        assert all(a.tobytes() == b.tobytes() for a, b in zip(o[:4], before[:4])), (entry, what)
        assert o[4].tobytes() == _outs(w, n)[4].tobytes(), (entry, what)


def test_single_winner_is_rank_0(world):
    """the six entries agree where they overlap: rank 0 of the ranked calls is the single-winner call's result
    (groups of two rows leave rank 0 as it is), and the knn calls on the index's own lists equal the fused ones"""
    w = world
    got = {}
    for entry in ENTRIES:
        o = _outs(w, N_BEST if topn(entry) else 1)
        assert _call(w, entry, o)[0] == OK, w['L'].asl_last_error()
        got[entry] = o
    one = got['asl_search_batch']
    for entry in ENTRIES[1:]:
        o = got[entry]
        assert np.array_equal(o[0][:, 0], one[0][:, 0]) and np.array_equal(o[1][:, 0], one[1][:, 0]), entry
        assert np.array_equal(o[2], one[2]) and np.array_equal(o[3][:, 0], one[3][:, 0]), entry
        assert np.array_equal(o[4][:, 0], one[4][:, 0]), entry
