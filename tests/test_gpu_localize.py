"""asl_localize_batch (csrc/localize.hip) against the numpy restatement tests/localize_ref.py, bit for bit,
and the localisation of open-search identifications through the engine."""
import ctypes as C
import functools
import itertools
import logging
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import localize_cases as LC     # noqa: E402
import localize_ref as R        # noqa: E402
from fake_reader import FakeReader, FakeSpectrum   # noqa: E402

OUT_DTYPES = tuple((k, np.float64 if k.endswith('score') else np.int32) for k in LC.SITE_KEYS + LC.SSM_KEYS)


def call_host(packed, tol, unit, fill=0, skip=()):
    """The C entry on host arrays: (return code, outputs). ``fill`` pre-sets the outputs."""
    from ann_solo_amd import _lib
    q, seq, mass, nterm, cterm, zmax, delta = packed
    out = {k: np.full(int(seq[-1]) if k in LC.SITE_KEYS else q.n, fill, dt) for k, dt in OUT_DTYPES}
    rc = _lib.lib().asl_localize_batch(
        C.byref(_lib.peaks_struct(q)), _lib.ptr(seq), _lib.ptr(mass), _lib.ptr(nterm), _lib.ptr(cterm),
        _lib.ptr(zmax), _lib.ptr(delta), float(tol), {'Da': 0, 'ppm': 1}.get(unit, unit),
        *[None if k in skip else _lib.ptr(out[k]) for k, _ in OUT_DTYPES])
    return rc, out


def call_device(packed, tol, unit):
    from ann_solo_amd import localize as lz
    return {k: v.cpu().numpy() for k, v in lz.localize_batch(*packed, tol, unit, 'cuda').items()}


# ---------------------------------------------------------------------------------------- the grid
LENGTHS = (2, 3, 17, 64, 65, 128)
CHARGES = (1, 2, 8)
PEAKS = (0, 1, 50, 256, 257, 1024, 4096)
TOLERANCES = ((0.02, 'Da'), (10.0, 'ppm'), (20000.0, 'ppm'), (0.0, 'Da'))
GRID_DELTAS = (15.994915, -17.026549, 0.0, 1e-9, 500.0, -150.0)      # -150: low fragments fall below m/z 0
N_PARTS = 3


@functools.lru_cache(maxsize=None)
def grid_batch(ti, part):
    """A third of the 126 (L, charge, peaks) combinations, shuffled so that one call mixes the lengths and
    the peak counts (wave packing, the second pass of L > 64, staged and unstaged spectra side by side), at
    tolerance ``TOLERANCES[ti]``; the deltas rotate, some peptides have terminal additions."""
    tol, unit = TOLERANCES[ti]
    rng = np.random.default_rng(100 * ti + part)
    combos = list(itertools.product(LENGTHS, CHARGES, PEAKS))
    order = np.random.default_rng(5).permutation(len(combos))
    cases = []
    for s, c in enumerate(order[part::N_PARTS]):
        L, z, n = combos[c]
        nterm, cterm = ((42.010565, 0.0), (0.0, -0.984016), (0.0, 0.0))[min(s % 7, 2)]
        cases.append(LC.random_case(rng, L, z, n, max(tol, 0.01) if unit == 'Da' else tol, unit,
                                    GRID_DELTAS[(s + ti + part) % len(GRID_DELTAS)], nterm, cterm))
    return cases, LC.reference(cases, tol, unit)


@pytest.mark.parametrize('part', range(N_PARTS))
@pytest.mark.parametrize('ti', range(len(TOLERANCES)))
def test_bit_identity_with_the_reference(ti, part):
    tol, unit = TOLERANCES[ti]
    cases, refs = grid_batch(ti, part)
    assert len(cases) == 42
    packed = LC.pack_cases(cases)
    LC.assert_same(call_device(packed, tol, unit), refs, packed[1], (tol, unit, part))
    hits = sum(int(r['site_count'].max()) for r in refs)
    print('tolerance', tol, unit, 'part', part, ': hits of the best-covered sites', hits)
    assert hits > 0 or tol == 0.0


# ---------------------------------------------------------------------------------------- window edges
def _edge_peptide():
    """Residue masses and an N-terminal addition for which theo(b_1, z = 1) is exactly 100.0: with R = 0.5
    both window edges are float32 values."""
    masses = np.array([50.0, 71.037114, 87.032028, 97.052764, 128.094963])
    nterm = np.float64(100.0) - R.PROTON - 50.0
    for _ in range(8):
        theo = (nterm + masses[0]) / np.float64(1.0) + R.PROTON
        if theo == 100.0:
            return masses, float(nterm)
        nterm = np.nextafter(nterm, np.inf if theo < 100.0 else -np.inf)
    raise AssertionError('no N-terminal addition gives theo = 100.0')


@pytest.mark.parametrize('unit,tol', (('Da', 0.5), ('ppm', 5000.0), ('Da', 0.02), ('ppm', 10.0)))
def test_window_edges(unit, tol):
    """One single-peak spectrum per planted value: the float32 values on either side of theo - R and
    theo + R and the nearest float32 of the edge itself, for b_1 (plain), y_2 (shifted) and b_3 at charge
    2. Whether the peak matches must be what the reference says; at R = 0.5 Da around theo = 100.0 the edges
    are representable and, being inclusive, match while their outer neighbours do not."""
    masses, nterm = _edge_peptide()
    delta, zmax = 15.994915, 2
    theo = R.fragment_theo(masses, nterm, 0.0, delta, zmax)
    cases, planted = [], []
    for (t, k, v, z) in ((0, 1, 0, 1), (1, 2, 1, 1), (0, 3, 0, 2)):
        th = theo[t, k, v, z - 1]
        reach = np.float64(tol) if unit == 'Da' else (np.float64(tol) * np.float64(1e-6)) * th
        for edge in (th - reach, th + reach):
            f = np.float32(edge)
            for x in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
                cases.append(LC.case(masses, [x], [3.0], delta, zmax, nterm))
                planted.append(((t, k, v, z), float(edge), float(x)))
    refs = LC.reference(cases, tol, unit)
    packed = LC.pack_cases(cases)
    out = call_device(packed, tol, unit)
    LC.assert_same(out, refs, packed[1], (unit, tol))
    matched = [bool(r['pick'][t, k, v, z - 1] >= 0) for r, ((t, k, v, z), _, _) in zip(refs, planted)]
    assert any(matched) and not all(matched)
    if (unit, tol) == ('Da', 0.5):
        assert theo[0, 1, 0, 0] == 100.0
        assert matched[:6] == [False, True, True, True, True, False]      # 99.5-, 99.5, 99.5+, 100.5-, 100.5, 100.5+


# ---------------------------------------------------------------------------------------- ties, multiplicity
def test_ties_and_multiplicity():
    pep = LC.parse('ACDEFGHIK')
    m = pep.masses
    delta, tol = 15.994915, 0.02
    theo = R.fragment_theo(m, 0.0, 0.0, delta, 2)
    b3, y4s = theo[0, 3, 0, 0], theo[1, 4, 1, 0]
    f = np.float32
    cases = [
        LC.case(m, [b3 - 0.01, b3 + 0.01], [2.0, 2.0], delta, 2),                   # two equal: the first
        LC.case(m, [b3 - 0.01, b3 + 0.01], [2.0, 5.0], delta, 2),                   # two unequal: the larger
        LC.case(m, [b3 - 0.01, b3, b3 + 0.01], [4.0, 4.0, 4.0], delta, 2),          # three equal
        LC.case(m, [b3 - 0.01, b3, b3 + 0.01], [1.0, 4.0, 4.0], delta, 2),          # the first of the largest
        LC.case(m, [b3 - 0.01, b3, b3 + 0.01], [1.0, 2.0, 7.0], delta, 2),
        LC.case(m, [f(b3), f(b3), f(b3)], [3.0, 3.0, 9.0], delta, 2),               # duplicate m/z
        LC.case(m, [f(y4s), f(y4s)], [6.0, 6.0], delta, 2),
        LC.case(m, [b3 + 0.005], [2.5], 0.01, 2),             # one peak, plain and shifted fragment (delta 0.01)
        # one peak for both charges of b_1: its base is 0.01, so theo is 1.0173 at z = 1 and 1.0123 at z = 2
        LC.case(m, [1.015], [1.5], delta, 2, nterm=0.01 - m[0]),
    ]
    refs = LC.reference(cases, tol, 'Da')
    assert [int(r['pick'][0, 3, 0, 0]) for r in refs[:6]] == [0, 1, 0, 1, 2, 2]
    assert refs[6]['pick'][1, 4, 1, 0] == 0
    assert refs[7]['pick'][0, 3, 0, 0] == 0 and refs[7]['pick'][0, 3, 1, 0] == 0
    assert refs[8]['pick'][0, 1, 0].tolist() == [0, 0] and refs[8]['none_score'] == 3.0
    packed = LC.pack_cases(cases)
    out = call_device(packed, tol, 'Da')
    LC.assert_same(out, refs, packed[1])
    assert out['none_score'].tolist() == [2.0, 5.0, 4.0, 4.0, 7.0, 9.0, 0.0, 2.5, 3.0]


# ---------------------------------------------------------------------------------------- nullable outputs
def test_nullable_outputs_and_pointer_kinds():
    rng = np.random.default_rng(4)
    cases = [LC.random_case(rng, L, z, n, 0.05, 'Da', d) for L, z, n, d in
             ((9, 2, 60, 15.994915), (70, 1, 300, -17.026549), (2, 3, 0, 79.966331))]
    refs = LC.reference(cases, 0.05, 'Da')
    packed = LC.pack_cases(cases)
    rc, full = call_host(packed, 0.05, 'Da', fill=77)
    assert rc == 0
    LC.assert_same(full, refs, packed[1], 'host pointers')
    LC.assert_same(call_device(packed, 0.05, 'Da'), refs, packed[1], 'device pointers')
    names = [k for k, _ in OUT_DTYPES]
    for mask in range(1, 1 << len(names)):
        skip = tuple(k for b, k in enumerate(names) if mask >> b & 1)
        rc, out = call_host(packed, 0.05, 'Da', fill=77, skip=skip)
        assert rc == 0, skip
        for k in names:
            if k in skip:
                assert np.all(out[k] == 77), (skip, k)
            else:
                assert np.array_equal(out[k].view(np.uint8), full[k].view(np.uint8)), (skip, k)


# ---------------------------------------------------------------------------------------- refusals
def test_limits_and_bad_arguments_write_nothing():
    """Each limit and bad argument of the header: its error code, outputs untouched. All of them are host
    checks before any launch."""
    from ann_solo_amd import _lib
    rng = np.random.default_rng(6)
    INVALID, CAPACITY = -1, -4

    def good():
        return [LC.random_case(rng, 9, 2, 50, 0.05, 'Da', 15.994915), LC.random_case(rng, 12, 1, 70, 0.05, 'Da', 42.010565)]

    def check(cases, want, tol=0.05, unit='Da'):
        rc, out = call_host(LC.pack_cases(cases), tol, unit, fill=77)
        assert rc == want, (rc, want, _lib.lib().asl_last_error())
        assert _lib.lib().asl_last_error()
        for k, v in out.items():
            assert np.all(v == 77), k
    rc, out = call_host(LC.pack_cases(good()), 0.05, 'Da', fill=77)
    assert rc == 0 and not np.all(out['site_score'] == 77) and not np.any(out['best_lo'] == 77)
    c = good()
    c[1] = LC.random_case(rng, 9, 2, 4097, 0.05, 'Da', 15.994915)
    check(c, CAPACITY)
    long = LC.random_case(rng, 128, 2, 10, 0.05, 'Da', 15.994915)
    long.update(L=129, masses=np.append(long['masses'], 57.021464))
    check(good() + [long], CAPACITY)
    c = good()
    c[0]['zmax'] = 9
    check(c, CAPACITY)
    c = good()
    c[0]['zmax'] = 0
    check(c, INVALID)
    one = LC.random_case(rng, 2, 2, 10, 0.05, 'Da', 15.994915)
    one.update(L=1, masses=one['masses'][:1])
    check(good() + [one], INVALID)
    for bad in (np.nan, np.inf):
        c = good()
        c[1]['masses'] = c[1]['masses'].copy()
        c[1]['masses'][5] = bad
        check(c, INVALID)
        for key, sign in (('nterm', 1), ('cterm', -1), ('delta', 1)):
            c = good()
            c[0][key] = sign * bad
            check(c, INVALID)
    check(good(), INVALID, tol=-1e-9)
    check(good(), INVALID, tol=np.nan)
    check(good(), INVALID, unit=2)


# ---------------------------------------------------------------------------------------- through the engine
N_LIB, N_MOD, N_PLAIN, N_NEAR = 300, 60, 20, 6
UNKNOWN_ROW = 7                 # its peptide names a modification nobody knows


def _engine_data(seed=31):
    """Library spectra: complete singly charged b / y ladders of random peptides of 8 .. 16 residues at
    precursor charge 2, some with ``C[Carbamidomethyl]``. Queries: N_MOD library spectra with one of the
    five masses on a known residue and the precursor moved with it, N_PLAIN unmodified copies, and N_NEAR
    copies whose precursor is off by 0.015 Da: outside the standard window, under the shift gate."""
    rng = np.random.default_rng(seed)
    specs, peps, inten = [], [], []
    for i in range(N_LIB):
        L = int(rng.integers(8, 17))
        text = LC.DC.random_peptide(rng, L, mod_p=0.05)
        if i % 5 == 0:
            text = 'C[Carbamidomethyl]' + text
        pep = LC.parse(text)
        if i == UNKNOWN_ROW:
            text = text[0] + '[Nope]' + text[1:] if text[1] != '[' else text.replace('[', '[Nope][', 1)
        b, y = LC.ladder_mz(pep.masses, 0, 0.0)
        it = rng.lognormal(0.0, 0.5, len(b) + len(y))
        pmz = (float(pep.masses.sum()) + R.H2O + 2 * R.PROTON) / 2
        order = np.argsort(np.concatenate((b, y)))
        specs.append(FakeSpectrum(f'lib{i:04d}', float(pmz), 2, np.concatenate((b, y))[order], it[order], None, text))
        peps.append(pep)
        inten.append(it)
    queries, truth = [], {}
    rows = rng.permutation(N_LIB)
    rows = np.concatenate(([UNKNOWN_ROW], rows[rows != UNKNOWN_ROW]))
    for j, i in enumerate(rows[:N_MOD + N_PLAIN + N_NEAR]):
        pep, pmz = peps[i], specs[i].precursor_mz
        if j < N_MOD:
            delta, site = LC.DELTAS[j % len(LC.DELTAS)], int(rng.integers(0, len(pep.sequence)))
        else:
            delta, site = (0.0 if j < N_MOD + N_PLAIN else 0.015), 0
        b, y = LC.ladder_mz(pep.masses, site, delta if j < N_MOD else 0.0)
        mz = np.concatenate((b, y)) + rng.normal(0.0, 0.002, len(b) + len(y))
        order = np.argsort(mz)
        queries.append(FakeSpectrum(f'scan={j}', float(pmz + delta / 2), 2, mz[order], inten[i][order], index=j))
        truth[f'scan={j}'] = (f'lib{i:04d}', delta, site, 'mod' if j < N_MOD else 'plain' if delta == 0.0 else 'near')
    return specs, queries, truth


def _search(tmp_path, specs, queries, localize):
    from ann_solo_amd.config import Config
    from ann_solo_amd.library_store import pack_queries
    from ann_solo_amd.spectral_library import SpectralLibrary
    cfg = Config.open_search(num_list=4, num_probe=4, num_candidates=64, kmeans_niter=4, min_mz_range=100.0,
                             precursor_tolerance_mass=5.0, precursor_tolerance_mode='ppm',
                             fragment_mz_tolerance=0.02, localize_modifications=localize)
    sl = SpectralLibrary(FakeReader(specs, str(tmp_path / 'lib.splib')), config=cfg, device='cuda:0')
    qs, qm = pack_queries(iter(queries), cfg, 'cuda:0')
    table = sl.search(qs, qm, sl.library_meta)
    return sl, qs, table


def test_through_the_engine(tmp_path, caplog):
    from ann_solo_amd.decoy_generator import default_fragment_charge
    specs, queries, truth = _engine_data()
    with caplog.at_level(logging.WARNING):
        sl, qs, on = _search(tmp_path, specs, queries, True)
    skipped = [r for r in caplog.records if 'localisation skipped' in r.getMessage()]
    assert len(skipped) == 1 and 'skipped 1 SSMs' in skipped[0].getMessage() and 'Nope' in skipped[0].getMessage()
    assert len(on) >= N_MOD + N_PLAIN                      # the search completed
    delta = on.mass_diffs()
    o, mz, it, *_ = qs[2].numpy()
    meta = sl.library_meta[2]
    n_loc = n_site = 0
    kinds = {'mod': 0, 'plain': 0, 'near': 0}
    for i in range(len(on)):
        qid = on.query_meta[2][int(on.qrow[i])]['identifier']
        lib_id, planted, site, kind = truth[qid]
        rec = meta[int(on.lib_row[i])]
        kinds[kind] += 1
        cols = (on.mod_mass[i], on.mod_site_lo[i], on.mod_site_hi[i], on.mod_site_score[i], on.mod_site_margin[i],
                on.mod_site_gain[i])
        localised = bool(on.open_level[i]) and abs(delta[i]) >= 0.02 and 'Nope' not in rec['peptide']
        if kind == 'plain':
            assert not on.open_level[i] and rec['identifier'] == lib_id
        if kind == 'near':
            assert on.open_level[i] and abs(delta[i]) < 0.02
        if not localised:
            assert np.isnan(cols[0]) and cols[1] == cols[2] == -1 and np.isnan(cols[3:]).all(), (qid, cols)
            continue
        n_loc += 1
        pep = LC.parse(rec['peptide'])
        a, b = int(o[on.qrow[i]]), int(o[on.qrow[i] + 1])
        r = R.localize_ref(mz[a:b], it[a:b], pep.masses, pep.nterm, pep.cterm, default_fragment_charge(2), delta[i],
                           0.02, 'Da')
        want = (delta[i], r['best_lo'], r['best_hi'], r['best_score'], r['best_score'] - r['runner_score'],
                r['best_score'] - r['none_score'])
        assert cols[1] == want[1] and cols[2] == want[2], (qid, cols, want)
        assert LC.bits([cols[0], *cols[3:]]).tolist() == LC.bits([want[0], *want[3:]]).tolist(), (qid, cols, want)
        s = on[i]
        assert (s.mod_site_lo, s.mod_site_hi, s.mod_site_score) == (want[1], want[2], want[3])
        if kind == 'mod' and rec['identifier'] == lib_id:
            n_site += 1
            assert abs(delta[i] - planted) < 1e-3
            assert cols[1] <= site <= cols[2], (qid, site, cols)
            assert cols[5] > 0.0
    print('SSMs', len(on), kinds, 'localised', n_loc, 'of them at their own peptide', n_site)
    # (how often the shifted dot product finds the query's own peptide is the search's business: most of them)
    assert kinds['plain'] == N_PLAIN and kinds['near'] >= 1 and n_site >= 0.8 * (N_MOD - 1)
    sl.shutdown()
    # the switch off: the same identifications, nothing localised
    sl2, _, off = _search(tmp_path, specs, queries, False)
    assert len(off) == len(on)
    for k in ('charge', 'qrow', 'lib_row', 'open_level'):
        assert np.array_equal(getattr(on, k), getattr(off, k)), k
    assert np.array_equal(LC.bits(on.score), LC.bits(off.score)) and np.array_equal(LC.bits(on.q), LC.bits(off.q))
    for i in range(len(on)):
        assert np.array_equal(on._peak_matches(i), off._peak_matches(i))
    assert np.isnan(off.mod_mass).all() and (off.mod_site_lo == -1).all() and (off.mod_site_hi == -1).all()
    assert np.isnan(off.mod_site_score).all() and np.isnan(off.mod_site_margin).all() and np.isnan(off.mod_site_gain).all()
    sl2.shutdown()
