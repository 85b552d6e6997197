"""asl_deplete_batch (csrc/deplete.hip) against the numpy restatement tests/deplete_ref.py, bit for bit, its
tie to the rescoring's peak matches, and the chimeric level through the engine."""
import ctypes as C
import functools

import numpy as np
import pytest

import deplete_cases as DC
import deplete_ref as R

pytestmark = pytest.mark.gpu

KEYS = ('mz', 'intensity', 'src', 'count', 'valid', 'kept_energy')
DTYPES = dict(mz=np.float32, intensity=np.float32, src=np.int32, count=np.int32, valid=np.uint8, kept_energy=np.float32)
INVALID, CAPACITY = -1, -4
SHIFT, PPM = R.SCORE_SHIFT, R.SCORE_FRAGMENT_PPM


def call(queries, library, rows, tol, flags, min_peaks, min_range, stride=None, device=False, skip=(), fill=None):
    """The C entry on host arrays, or (``device``) on device tensors: (return code, outputs as numpy; None for
    the outputs in ``skip``, which are passed as NULL). ``fill`` pre-sets the outputs."""
    import torch
    from ann_solo_amd import _lib
    n = len(queries[0]) - 1
    if stride is None:
        stride = int(np.diff(queries[0]).max()) if n else 0
    out = {k: np.full((n, stride) if k in KEYS[:3] else n, 0 if fill is None else fill, DTYPES[k]) for k in KEYS}
    rows = np.ascontiguousarray(rows, np.int64)
    if device:
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')
        queries, library = tuple(dev(a) for a in queries), tuple(dev(a) for a in library)
        rows, held = dev(rows), {k: dev(v) for k, v in out.items()}
    else:
        held = out
    rc = _lib.lib().asl_deplete_batch(
        C.byref(_lib.peaks_struct(queries)), C.byref(_lib.peaks_struct(library)), _lib.ptr(rows), float(tol),
        int(flags), int(min_peaks), float(min_range), int(stride),
        *[None if k in skip else _lib.ptr(held[k]) for k in KEYS])
    if device:
        out = {k: v.cpu().numpy() for k, v in held.items()}
    return rc, {k: (None if k in skip else v) for k, v in out.items()}


def assert_same(got, ref, what):
    for k in KEYS:
        if got[k] is None:
            continue
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k].astype(DTYPES[k]))
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a.view(np.uint8 if a.itemsize == 1 else np.uint32) !=
                              b.view(np.uint8 if b.itemsize == 1 else np.uint32))
            raise AssertionError(f'{what}: {k} differs at {bad[:5].tolist()}: {a[tuple(bad[0])]} != {b[tuple(bad[0])]}')


# ---------------------------------------------------------------------------------------- the grid
MIN_PEAKS, MIN_RANGE = 10, 250.0


@functools.lru_cache(maxsize=None)
def grid(fi):
    """The batch of DC.grid_batch(fi), packed, some SSMs skipped, and its reference -- computed once."""
    ssms = DC.grid_batch(fi)
    q, lib, rows = DC.pack(ssms, skip=(3, 40, len(ssms) - 1))
    ref = R.deplete_batch(q, lib, rows, DC.tol_of(DC.FLAGS[fi]), DC.FLAGS[fi], MIN_PEAKS, MIN_RANGE)
    return ssms, q, lib, rows, ref


@pytest.mark.parametrize('fi', range(len(DC.FLAGS)))
def test_bit_identity_with_the_reference(fi):
    """102 SSMs per flag word: every (query peaks, library peaks) pair of the grid, every charge against every
    precursor difference; host pointers, device pointers, and out_src / kept_energy NULL."""
    flags = DC.FLAGS[fi]
    ssms, q, lib, rows, ref = grid(fi)
    assert len(ssms) == len(DC.Q_PEAKS) * len(DC.L_PEAKS) + len(DC.CHARGES) * len(DC.PMD_KINDS)
    tol = DC.tol_of(flags)
    for device, skip in ((False, ()), (True, ()), (fi % 2 == 0, ('src', 'kept_energy'))):
        rc, out = call(q, lib, rows, tol, flags, MIN_PEAKS, MIN_RANGE, device=device, skip=skip, fill=0x55)
        assert rc == 0, rc
        assert_same(out, ref, (flags, device, skip))
    kept, total = int(ref['count'].sum()), int(np.diff(q[0]).sum())
    print('flags', flags, ': kept', kept, 'of', total, 'peaks; valid residues', int(ref['valid'].sum()))
    assert 0.2 * total < kept < 0.9 * total and 0 < ref['valid'].sum() < len(ssms)
    # the padding is zero, the skipped rows are empty
    for s in (3, 40, len(ssms) - 1):
        assert out['count'][s] == 0 and out['valid'][s] == 0 and not out['mz'][s].any()
    slot = np.arange(out['mz'].shape[1])[None, :] >= out['count'][:, None]
    assert not out['mz'][slot].any() and not out['intensity'][slot].any()


@pytest.mark.parametrize('flags', (SHIFT, SHIFT | PPM))
def test_library_without_annotation(flags):
    """library->charge == NULL is every charge 0; an unannotated library says the same with an array."""
    rng = np.random.default_rng(9)
    ssms = [DC.make_ssm(rng, qn, ln, z, kind, flags, 'none')
            for qn, ln in ((65, 50), (300, 257), (50, 300)) for z in (1, 3, 31) for kind in DC.PMD_KINDS[2:]]
    q, lib, rows = DC.pack(ssms, lib_charge=False)
    zeros = lib[:3] + (np.zeros(len(lib[1]), np.uint8),) + lib[4:]
    tol = DC.tol_of(flags)
    ref = R.deplete_batch(q, zeros, rows, tol, flags, MIN_PEAKS, MIN_RANGE)
    for library, device in ((lib, False), (lib, True), (zeros, False)):
        rc, out = call(q, library, rows, tol, flags, MIN_PEAKS, MIN_RANGE, device=device)
        assert rc == 0
        assert_same(out, ref, (flags, device))
    assert 0 < ref['count'].sum() < np.diff(q[0]).sum()


# ---------------------------------------------------------------------------------------- window edges
@pytest.mark.parametrize('unit,tol', (('Da', 0.5), ('ppm', 5000.0), ('Da', 0.02), ('ppm', 10.0)))
def test_window_edges(unit, tol):
    """Single-peak queries on the float32 values around x - tol_i and x + tol_i, for the library peak itself
    (x = 100) and for its c = 1 and c = 2 shifted positions: explained or not is what the reference says; at
    0.5 Da around 100.0 the edges are representable and, being inclusive, explain, while their outer neighbours
    do not."""
    flags = R.flags_of(True, unit)
    z, l_pmz, q_pmz = 2, 600.0, 608.0            # pmd = 16: positions 100, 116 (c = 1), 108 (c = 2)
    ssms, planted = [], []
    for x, chg in ((100.0, 0), (116.0, 1), (108.0, 2), (116.0, 2)):
        # (ppm: the window is relative to the QUERY peak q, |q - x| <= rel q: its edges are x / (1 +- rel))
        rel = tol * 1e-6
        for edge in ((x - tol, x + tol) if unit == 'Da' else (x / (1.0 + rel), x / (1.0 - rel))):
            f = np.float32(edge)
            around = [f]
            for _ in range(2):
                around = [np.nextafter(around[0], np.float32(-np.inf))] + around + \
                         [np.nextafter(around[-1], np.float32(np.inf))]
            for v in around:
                ssms.append(dict(q_mz=np.array([v], np.float32), q_int=np.ones(1, np.float32), q_pmz=q_pmz,
                                 l_mz=np.array([100.0], np.float32), l_int=np.ones(1, np.float32),
                                 l_chg=np.array([chg], np.uint8), l_pmz=l_pmz, z=z))
                planted.append((x, chg, float(v)))
    q, lib, rows = DC.pack(ssms)
    ref = R.deplete_batch(q, lib, rows, tol, flags, 1, 0.0)
    rc, out = call(q, lib, rows, tol, flags, 1, 0.0)
    assert rc == 0
    assert_same(out, ref, (unit, tol))
    explained = (ref['count'] == 0).reshape(4, 2, 5)
    assert explained[:3].any() and not explained[:3].all()
    assert not explained[3].any()                # a peak annotated 2+ never shifts by pmd / 1
    if (unit, tol) == ('Da', 0.5):
        for k in range(3):
            assert explained[k, 0].tolist() == [False, False, True, True, True], k      # .. 99.5-, 99.5, 99.5+ ..
            assert explained[k, 1].tolist() == [True, True, True, False, False], k


# ---------------------------------------------------------------------------------------- validity edges
def test_validity_edges():
    """Kept count equal to min_peaks and one below; kept span equal to min_mz_range and one float32 below. The
    library row explains the two outermost peaks of every query, so the edges are those of the KEPT peaks."""
    below = np.nextafter(np.float32(450.0), np.float32(0.0))
    ssms = []
    for n, last in ((10, 450.0), (9, 450.0), (10, below), (11, 450.0), (11, below)):
        inner = np.concatenate([[200.0], np.linspace(210.0, 440.0, n - 2), [last]]).astype(np.float32)
        q_mz = np.concatenate([[100.0], inner, [900.0]]).astype(np.float32)
        ssms.append(dict(q_mz=q_mz, q_int=np.linspace(0.2, 1.0, len(q_mz)).astype(np.float32), q_pmz=500.0,
                         l_mz=np.array([100.0, 900.0], np.float32), l_int=np.ones(2, np.float32),
                         l_chg=np.zeros(2, np.uint8), l_pmz=500.0, z=2))
    q, lib, rows = DC.pack(ssms)
    ref = R.deplete_batch(q, lib, rows, 0.02, 0, 10, 250.0)
    assert ref['count'].tolist() == [10, 9, 10, 11, 11] and ref['valid'].tolist() == [1, 0, 0, 1, 0]
    for device in (False, True):
        rc, out = call(q, lib, rows, 0.02, 0, 10, 250.0, device=device)
        assert rc == 0
        assert_same(out, ref, device)


# ---------------------------------------------------------------------------------------- refusals
def test_limits_and_bad_arguments_write_nothing():
    """Each limit and bad argument of the header: its error code, outputs untouched. All of them are host
    checks before any launch."""
    from ann_solo_amd import _lib
    rng = np.random.default_rng(6)

    def good(qn=(40, 70), ln=(30, 50)):
        return [DC.make_ssm(rng, a, b, 2, 15.994915, SHIFT) for a, b in zip(qn, ln)]

    def check(ssms, want, tol=0.02, flags=SHIFT, stride=None, rows=None):
        q, lib, r = DC.pack(ssms)
        rc, out = call(q, lib, r if rows is None else rows, tol, flags, 10, 250.0, stride=stride, fill=77)
        assert rc == want, (rc, want, _lib.lib().asl_last_error())
        assert _lib.lib().asl_last_error()
        for k, v in out.items():
            assert np.all(v == 77), k
    q, lib, r = DC.pack(good())
    rc, out = call(q, lib, r, 0.02, SHIFT, 10, 250.0, stride=80, fill=77)
    assert rc == 0 and not np.any(out['count'] == 77) and not np.any(out['mz'] == 77)      # every slot is written
    check(good(qn=(40, 4097)), CAPACITY)
    check(good(ln=(4097, 50)), CAPACITY)
    check(good(), CAPACITY, stride=69)
    check(good(), INVALID, tol=-1e-9)
    check(good(), INVALID, tol=np.nan)
    check(good(), INVALID, flags=4)
    check(good(), INVALID, flags=SHIFT | 8)
    check(good(), INVALID, rows=np.array([0, 2]))
    # a row of 4097 peaks that no SSM names is nobody's business
    q, lib, r = DC.pack(good(ln=(4097, 50)))
    r[int(np.argmax(np.diff(lib[0])[r]))] = -1
    rc, out = call(q, lib, r, 0.02, SHIFT, 10, 250.0)
    assert rc == 0 and sorted(out['count'].tolist())[0] == 0


# ---------------------------------------------------------------------------------------- tie to the search
@pytest.mark.parametrize('flags', DC.FLAGS)
def test_no_matched_peak_of_the_winner_survives(flags):
    """asl_rescore_batch with the single winning candidate, on the device, then the depletion: no query index of
    pm_pairs[:pm_count] is left in out_src. (Sizes and charges stay under the rescoring's 512 generated matches per
    pair: at the gate's edge every direct match is generated once per shift.)"""
    import torch
    from ann_solo_amd import _lib
    from ann_solo_amd.packed import PackedSpectra
    rng = np.random.default_rng(21 + flags)
    ssms = [DC.make_ssm(rng, qn, ln, z, kind, flags)
            for qn, ln in ((50, 50), (65, 64), (64, 256)) for z in DC.CHARGES[:5] for kind in DC.PMD_KINDS]
    q, lib, rows = DC.pack(ssms)
    tol, n = DC.tol_of(flags), len(ssms)
    Q, L = PackedSpectra.from_numpy(*q, device='cuda:0'), PackedSpectra.from_numpy(*lib, device='cuda:0')
    d_rows = torch.from_numpy(rows).to('cuda:0')
    offs = torch.arange(n + 1, dtype=torch.int32, device='cuda:0')
    best = torch.full((n,), -7, dtype=torch.int32, device='cuda:0')
    score = torch.zeros(n, dtype=torch.float64, device='cuda:0')
    count = torch.zeros(n, dtype=torch.int32, device='cuda:0')
    pairs = torch.zeros((n, 256, 2), dtype=torch.int32, device='cuda:0')
    _lib.check(_lib.lib().asl_rescore_batch(C.byref(_lib.peaks_struct(Q)), C.byref(_lib.peaks_struct(L)),
                                            _lib.ptr(d_rows), _lib.ptr(offs), tol, flags, _lib.ptr(best),
                                            _lib.ptr(score), _lib.ptr(count), _lib.ptr(pairs), 256))
    rc, out = call(q, lib, rows, tol, flags, 1, 0.0, device=True)
    assert rc == 0
    count, pairs = count.cpu().numpy(), pairs.cpu().numpy()
    assert (best.cpu().numpy() == 0).all() and count.sum() > 5 * n
    for s in range(n):
        matched = set(pairs[s, :count[s], 0].tolist())
        assert not matched & set(out['src'][s, :out['count'][s]].tolist()), s
    assert out['count'].sum() > n


# ---------------------------------------------------------------------------------------- through the engine
def _launches(name):
    from ann_solo_amd import _lib
    ms, n = C.c_double(), C.c_int64()
    _lib.lib().asl_profile_get(name.encode(), C.byref(ms), C.byref(n))
    return n.value


@pytest.mark.parametrize('isolation', (False, True))
def test_through_the_engine(O, isolation):
    """The planted world of the CPU test through the real engine: the table of the reference pipeline (the
    engine's own table with the switch off, then tests/deplete_ref.py and the oracle's dot product on the
    residues) -- rows, ranks, scores to the bit, explained_intensity. With isolation windows on every query the
    intervals come from the metadata: the partner 2.0 m/z away is found then, and only then. Switch off: no
    depletion launch, today's table."""
    from ann_solo_amd import _lib, spectrum_similarity
    from ann_solo_amd.config import Config
    from ann_solo_amd.spectral_library import SpectralLibrary
    lib, qs, qmeta, lmeta, kw, plan = DC.world(isolation)
    engines = []
    L = _lib.lib()
    try:
        tables = {}
        for on in (False, True):
            sl = SpectralLibrary(lib, config=Config.open_search(chimeric_search=on, **kw))
            engines.append(sl)
            L.asl_profile_reset()
            L.asl_profile_enable(1)
            try:
                tables[on] = sl.search_packed(qs, qmeta, lmeta)
                sl.synchronize()
            finally:
                L.asl_profile_enable(0)
            assert (_launches('deplete') > 0) == on
        off, got = tables[False], tables[True]
        n0 = len(off)
        assert n0 >= DC.N_PLANTED and not off.chimeric_rank.any() and np.isnan(off.explained_intensity).all()
        for name in ('charge', 'qrow', 'lib_row', 'score', 'q', 'open_level', 'chimeric_rank', 'explained_intensity'):
            a, b = getattr(got, name)[:n0], getattr(off, name)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
        for i in range(n0):
            assert np.array_equal(got._peak_matches(i), off._peak_matches(i))
        ref = DC.reference_level(O, off, lib, qs, qmeta, lmeta, engines[1].config,
                                 cosines=spectrum_similarity.ssm_cosine)
        assert len(got) == n0 + len(ref) and len(ref) >= DC.N_PLANTED
        assert got.qrow[n0:].tolist() == [r[0] for r in ref] and got.lib_row[n0:].tolist() == [r[1] for r in ref]
        assert got.score[n0:].tobytes() == np.array([r[2] for r in ref]).tobytes()
        assert got.explained_intensity[n0:].tobytes() == np.array([r[3] for r in ref]).tobytes()
        assert (got.chimeric_rank[n0:] == 1).all() and not got.open_level[n0:].any()
        rank0 = {int(q): int(r) for q, r in zip(off.qrow, off.lib_row)}
        rank1 = {int(q): int(r) for q, r in zip(got.qrow[n0:], got.lib_row[n0:])}
        for i in range(DC.N_PLANTED):
            assert rank0[i] == plan[i][0] and rank1[i] == plan[i][1], i
        assert (rank1.get(DC.FAR) == plan[DC.FAR][1]) == isolation
        assert got[n0].chimeric_rank == 1 and got[0].chimeric_rank == 0
    finally:
        for sl in engines:
            sl.shutdown()
