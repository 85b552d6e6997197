"""asl_decoy_batch (csrc/decoy.hip) against the numpy restatement tests/decoy_ref.py, bit for bit, and
the decoy library end to end through the reader adapter."""
import ctypes as C
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import decoy_cases as DC     # noqa: E402
import decoy_ref as R        # noqa: E402
from fake_reader import FakeReader, FakeSpectrum   # noqa: E402

OUT_DTYPES = (('mz', np.float32), ('intensity', np.float32), ('src', np.int32), ('charge', np.uint8),
              ('ann_type', np.uint8), ('ann_n', np.uint8), ('ann_z', np.uint8), ('ann_loss', np.uint8))


def call_host(packed, tol, unit, fill=0, skip=()):
    """The C entry on host arrays: (return code, outputs). ``fill`` pre-sets the outputs."""
    from ann_solo_amd import _lib
    raw, seq, mass, perm, nterm, cterm, zmax = packed
    P = int(raw.mz.numel())
    out = {k: np.full(P, fill, dt) for k, dt in OUT_DTYPES}
    rc = _lib.lib().asl_decoy_batch(
        C.byref(_lib.peaks_struct(raw)), _lib.ptr(seq), _lib.ptr(mass), _lib.ptr(perm), _lib.ptr(nterm),
        _lib.ptr(cterm), _lib.ptr(zmax), float(tol), {'Da': 0, 'ppm': 1}.get(unit, unit),
        *[None if k in skip else _lib.ptr(out[k]) for k, _ in OUT_DTYPES])
    return rc, out


def call_device(packed, tol, unit):
    from ann_solo_amd import decoy_generator as dg
    out = dg.decoy_batch(*packed, tol, unit, 'cuda')
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_known_answer_of_the_reference():
    """Order and intensities exactly; |d m/z| <= 4e-5: half a float32 ulp below m/z 1024 (3.05e-5) plus
    the restatement's 9.7e-7 against the fixture's 8 decimals, rounded up."""
    from ann_solo_amd import decoy_generator as dg
    k = json.load(open(os.path.join(HERE, 'golden', 'decoy_kat.json')))
    pep = dg.parse_peptide(k['peptide'])
    case = dict(masses=pep.masses, perm=np.asarray(k['perm'], np.int32), nterm=0.0, cterm=0.0,
                zmax=dg.default_fragment_charge(k['precursor_charge']), charge=k['precursor_charge'],
                mz=np.asarray(k['mz'], np.float32), intensity=np.asarray(k['intensity'], np.float32), L=12)
    out = call_device(DC.pack_cases([case]), k['tolerance'], k['unit'])
    want_int = np.asarray(k['decoy_intensity'], np.float32)
    assert np.array_equal(out['intensity'], want_int)
    assert np.array_equal(case['intensity'][out['src']], want_int)
    d = np.abs(out['mz'].astype(np.float64) - np.asarray(k['decoy_mz']))
    print('max |dmz| against the fixture', d.max(), '; annotated peaks', int((out['ann_type'] > 0).sum()))
    assert d.max() <= 4e-5
    assert max(k['decoy_mz']) < 1024.0


SIZES = (0, 1, 63, 64, 65, 256, 257, 1025, 4096)
SMALL = (0, 1, 63, 64, 65, 256, 257)
CHARGES = (1, 2, 4, 7)
LENGTHS = (2, 3, 12, 33, 128)
TOL = {'Da': 0.05, 'ppm': 20.0}


@functools.lru_cache(maxsize=None)
def batch(L, unit):
    """40 spectra of peptides of L residues: every precursor charge, every peak count (the two large
    ones once, with a charge that rotates over the lengths), terminal additions on some, a negative
    modification on some; neighbours differ in size. The reference is computed once per batch."""
    rng = np.random.default_rng(1000 * L + (unit == 'ppm'))
    li = LENGTHS.index(L) + (unit == 'ppm')
    cases = []
    for s in range(40):
        n = SIZES[s] if s < len(SIZES) else SMALL[int(rng.integers(0, len(SMALL)))]
        Z = CHARGES[(s + li) % 4]
        cases.append(DC.make_case(rng, L, Z, n, TOL[unit], unit, nterm=42.010565 if s % 3 == 1 else 0.0,
                                  cterm=-0.984016 if s % 5 == 2 else 0.0, negative=s % 4 == 3))
    order = rng.permutation(40)
    cases = [cases[i] for i in order]
    return cases, DC.pack_cases(cases), DC.reference(cases, TOL[unit], unit)


@pytest.mark.parametrize('unit', ['Da', 'ppm'])
@pytest.mark.parametrize('L', LENGTHS)
def test_bit_exact_against_the_restatement(L, unit):
    cases, packed, refs = batch(L, unit)
    out = call_device(packed, TOL[unit], unit)
    off = packed[0].offsets.numpy()
    DC.assert_same(out, refs, off, (L, unit))
    # the data does exercise the annotation: peaks of every ion type found, most planted fragments hit
    if L >= 12:
        assert set(np.unique(out['ann_type']).tolist()) == {0, 1, 2, 3, 4}
        assert 0.3 < (out['ann_type'] > 0).mean() < 0.95
    # invariants: ascending output, intensity multiset kept, p peaks stay where they are
    for s, c in enumerate(cases):
        a, b = int(off[s]), int(off[s + 1])
        mz = out['mz'][a:b]
        assert np.all(np.diff(mz) >= 0)
        assert np.array_equal(np.sort(out['intensity'][a:b]), np.sort(c['intensity']))
        assert np.array_equal(np.sort(out['src'][a:b]), np.arange(b - a))
        is_p = out['ann_type'][a:b] == 3
        where = np.argsort(out['src'][a:b])          # decoy position of raw peak i
        assert np.array_equal(mz[where][is_p].view(np.uint32), c['mz'][is_p].view(np.uint32))
    # host arrays and nullable outputs give the same answer
    if L == 12:
        rc, host = call_host(packed, TOL[unit], unit, skip=('intensity', 'ann_n'))
        assert rc == 0
        for k in ('mz', 'src', 'charge', 'ann_type', 'ann_z', 'ann_loss'):
            assert np.array_equal(host[k], out[k]), k
        assert not host['intensity'].any() and not host['ann_n'].any()


@pytest.mark.parametrize('unit', ['Da', 'ppm'])
def test_ladders_that_do_not_rise_steadily(unit):
    """A residue lighter than 1e-3 Da or of negative mass: the kernel leaves its bisection for the
    exhaustive scan; a tolerance above 5e5 ppm does the same. Same bits as the restatement."""
    rng = np.random.default_rng(77)
    cases = [DC.make_case(rng, L, Z, n, TOL[unit], unit, light=True)
             for L, Z, n in ((3, 2, 40), (12, 3, 300), (12, 5, 65), (33, 4, 257), (7, 1, 64))]
    packed = DC.pack_cases(cases)
    out = call_device(packed, TOL[unit], unit)
    DC.assert_same(out, DC.reference(cases, TOL[unit], unit), packed[0].offsets.numpy(), unit)
    assert (out['ann_type'] > 0).any()
    if unit == 'ppm':
        wide = [DC.make_case(rng, 12, 3, 100, 20.0, 'ppm') for _ in range(3)]
        packed = DC.pack_cases(wide)
        for tol in (6e5, 2e6):
            DC.assert_same(call_device(packed, tol, 'ppm'), DC.reference(wide, tol, 'ppm'),
                           packed[0].offsets.numpy(), tol)


def _scan(case, x, tol, unit):
    """The annotation rule spelt out once more, fragment by fragment in Python: (type, n, z, loss) of the
    matching fragment of lowest theoretical m/z, first in (type, n, z, loss) order; None without a match."""
    ft, fn, fz, fl, base = R.fragment_table(case['masses'], case['nterm'], case['cterm'], case['zmax'])
    best = None
    for t, n, z, l, b in zip(ft.tolist(), fn.tolist(), fz.tolist(), fl.tolist(), base.tolist()):
        theo = (b + float(R.LOSSES[l])) / float(z) + R.PROTON
        reach = tol if unit == 'Da' else (tol * 1e-6) * theo
        if abs(float(x) - theo) <= reach and (best is None or theo < best[0]):
            best = (theo, t, n, z, l)
    return best


@pytest.mark.parametrize('unit', ['Da', 'ppm'])
def test_planted_edges(unit):
    tol = TOL[unit]
    rng = np.random.default_rng(9)
    case = DC.make_case(rng, 14, 4, 0, tol, unit)
    ft, fn, fz, fl, base = R.fragment_table(case['masses'], 0.0, 0.0, case['zmax'])
    theo = R.theo_of(base, fl, fz)
    order = np.argsort(theo, kind='stable')
    st = theo[order]
    reach = lambda t: tol if unit == 'Da' else (tol * 1e-6) * t
    peaks = []
    # (a) the edge of the window of fragments with no other fragment near: theo +- reach, and the float32
    #     values one and two ulps to either side
    lonely = [i for i in range(1, len(st) - 1) if st[i] > 150 and st[i] - st[i - 1] > 4 * reach(st[i]) and
              st[i + 1] - st[i] > 4 * reach(st[i])][:12]
    assert len(lonely) >= 6
    for i in lonely:
        for edge in (st[i] - reach(st[i]), st[i] + reach(st[i])):
            x = np.float32(edge)
            for _ in range(2):
                x = np.nextafter(x, np.float32(0))
            for _ in range(5):
                peaks.append(x)
                x = np.nextafter(x, np.float32(np.inf))
    # (b) a peak inside the windows of two fragments of different n: between them
    pairs = [(i, i + 1) for i in range(len(st) - 1)
             if 0 < st[i + 1] - st[i] < 0.8 * reach(st[i]) and fn[order[i]] != fn[order[i + 1]]][:10]
    assert len(pairs) >= 3, len(pairs)
    for i, j in pairs:
        peaks.append(np.float32(0.5 * (st[i] + st[j])))
    n_b = len(pairs)
    # (c) two peaks on the same new m/z: the same annotated raw m/z twice, and three times
    hit = np.float32(st[lonely[0]])
    peaks += [hit, hit, np.float32(st[lonely[1]])] + [np.float32(st[lonely[1]])] * 2
    mz = np.sort(np.asarray(peaks, np.float32), kind='stable')
    case.update(mz=mz, intensity=np.arange(1, len(mz) + 1, dtype=np.float32))
    packed = DC.pack_cases([case])
    out = call_device(packed, tol, unit)
    ref = DC.reference([case], tol, unit)
    DC.assert_same(out, ref, packed[0].offsets.numpy(), unit)
    inside = outside = both = 0
    for i, x in enumerate(mz):
        want = _scan(case, x, tol, unit)
        got = (int(out['ann_type'][i]), int(out['ann_n'][i]), int(out['ann_z'][i]), int(out['ann_loss'][i]))
        assert got == ((0, 0, 0, 0) if want is None else want[1:]), (i, x, got, want)
        inside += want is not None
        outside += want is None
        if want is not None:
            near = np.abs(np.float64(x) - theo) <= (tol if unit == 'Da' else (tol * 1e-6) * theo)
            if len(set(fn[near].tolist())) > 1:
                both += 1
                assert want[0] == theo[near].min()
    assert inside >= 20 and outside >= 20 and both >= n_b >= 3
    # equal new m/z: the raw order decides
    new = out['mz']
    for v in np.unique(new):
        src = out['src'][new == v]
        assert np.all(np.diff(src) > 0)
    assert (np.diff(new) == 0).sum() >= 3


def test_identity_permutation_returns_the_input():
    """a + (x - a) is exact where x - a is (Sterbenz): the decoy of the unshuffled peptide is the target."""
    rng = np.random.default_rng(4)
    cases = [DC.make_case(rng, L, Z, n, 20.0, 'ppm', identity=True)
             for L, Z, n in ((2, 2, 30), (12, 3, 257), (33, 4, 1025), (20, 2, 64))]
    packed = DC.pack_cases(cases)
    out = call_device(packed, 20.0, 'ppm')
    raw = packed[0]
    assert np.array_equal(out['mz'].view(np.uint32), raw.mz.numpy().view(np.uint32))
    assert np.array_equal(out['intensity'], raw.intensity.numpy())
    off = raw.offsets.numpy()
    assert np.array_equal(out['src'], np.concatenate([np.arange(off[s + 1] - off[s]) for s in range(raw.n)]))
    assert (out['ann_type'] > 0).mean() > 0.3 and np.array_equal(out['charge'], out['ann_z'])


def test_single_spectrum_call_and_batch_call_agree():
    """``shuffle_and_reposition(spectrum)``, the reference's call shape, is the batch call on one row; a
    row's decoy does not depend on the rows around it."""
    from ann_solo_amd import decoy_generator as dg
    from ann_solo_amd.library_store import pack_raw
    rng = np.random.default_rng(12)
    specs = []
    for i, (L, Z) in enumerate(((9, 2), (15, 3), (12, 2), (20, 4))):
        c = DC.make_case(rng, L, Z, 80, 0.02, 'Da')
        specs.append(FakeSpectrum(f'id{i}', 500.0 + i, Z, c['mz'], c['intensity'], None, c['peptide']))
    decoy, names, ann = dg.shuffle_and_reposition_batch(pack_raw(specs), [s.peptide for s in specs], 0.02, 'Da',
                                                        seed=3, device='cuda')
    assert decoy.identifiers == ['DECOY_id0', 'DECOY_id1', 'DECOY_id2', 'DECOY_id3']
    o, mz, it, chg, pmz, pz = decoy.numpy()
    assert np.array_equal(chg[np.argsort(o[:-1].repeat(80) + ann['src'].cpu().numpy(), kind='stable')],
                          ann['z'].cpu().numpy())
    for i, s in enumerate(specs):
        one = dg.shuffle_and_reposition(s, 0.02, 'Da', seed=3, device='cuda')
        assert one.identifier == 'DECOY_' + s.identifier and one.is_decoy is True
        assert one.precursor_mz == s.precursor_mz and one.precursor_charge == s.precursor_charge
        pep = dg.parse_peptide(s.peptide)
        _, perm = dg.shuffle(pep.sequence, dg.peptide_rng(3, s.peptide, s.precursor_charge))
        assert one.peptide == names[i] == str(pep.permuted(perm))
        assert sorted(dg.parse_peptide(one.peptide).masses.tolist()) == sorted(pep.masses.tolist())
        a, b = o[i], o[i + 1]
        assert np.array_equal(one.mz, mz[a:b]) and np.array_equal(one.intensity, it[a:b])
        assert np.array_equal(one.charge, chg[a:b])
        r = R.decoy_ref(s.mz, s.intensity, pep.masses, perm, 0.0, 0.0, max(1, s.precursor_charge - 1), 0.02, 'Da')
        assert np.array_equal(one.mz.view(np.uint32), r['mz'].view(np.uint32))
        other = dg.shuffle_and_reposition(s, 0.02, 'Da', seed=4, device='cuda')
        assert len(other.mz) == len(one.mz)
    with pytest.raises(ValueError, match='id0'):
        specs[0].peptide = 'PEPTIDE1K'
        dg.shuffle_and_reposition(specs[0], device='cuda')


def test_limits_and_bad_arguments_write_nothing():
    """Each limit and bad argument of the header: its error code, outputs untouched. All of them are host
    checks before any launch."""
    from ann_solo_amd import _lib
    rng = np.random.default_rng(6)
    INVALID, CAPACITY = -1, -4

    def good():
        return [DC.make_case(rng, 9, 3, 50, 0.05, 'Da'), DC.make_case(rng, 12, 2, 70, 0.05, 'Da')]

    def check(cases, want, tol=0.05, unit='Da', edit=None):
        packed = list(DC.pack_cases(cases))
        if edit:
            edit(packed)
        rc, out = call_host(tuple(packed), tol, unit, fill=77)
        assert rc == want, (rc, want, _lib.lib().asl_last_error())
        assert _lib.lib().asl_last_error()
        for k, v in out.items():
            assert np.all(v == 77), k
    rc, out = call_host(DC.pack_cases(good()), 0.05, 'Da', fill=77)
    assert rc == 0 and not np.all(out['mz'] == 77)
    c = good()
    c[1] = DC.make_case(rng, 9, 3, 4097, 0.05, 'Da')
    check(c, CAPACITY)
    long = DC.make_case(rng, 128, 2, 10, 0.05, 'Da')
    long.update(L=129, masses=np.append(long['masses'], 57.021464), perm=np.append(long['perm'], 128).astype(np.int32))
    check(good() + [long], CAPACITY)
    c = good()
    c[0]['zmax'] = 9
    check(c, CAPACITY)
    c = good()
    c[0]['zmax'] = 0
    check(c, INVALID)
    one = DC.make_case(rng, 2, 2, 10, 0.05, 'Da')
    one.update(L=1, masses=one['masses'][:1], perm=np.zeros(1, np.int32))
    check(good() + [one], INVALID)
    c = good()
    c[1]['perm'] = c[1]['perm'].copy()
    c[1]['perm'][3] = c[1]['perm'][4]                    # a repeated index
    check(c, INVALID)
    c = good()
    c[0]['perm'] = c[0]['perm'].copy()
    c[0]['perm'][0] = 9                                  # beyond the peptide
    check(c, INVALID)
    c = good()
    c[0]['perm'] = c[0]['perm'].copy()
    c[0]['perm'][0] = -1
    check(c, INVALID)
    for bad in (np.nan, np.inf):
        c = good()
        c[1]['masses'] = c[1]['masses'].copy()
        c[1]['masses'][5] = bad
        check(c, INVALID)
        c = good()
        c[0]['nterm'] = bad
        check(c, INVALID)
        c = good()
        c[0]['cterm'] = -bad
        check(c, INVALID)
    check(good(), INVALID, tol=-1e-9)
    check(good(), INVALID, tol=np.nan)
    check(good(), INVALID, unit=2)


# ---------------------------------------------------------------------------------------- end to end
def _library(n=300, seed=21):
    """Raw library spectra of random tryptic peptides: their own b / y / a fragments with small mass
    errors and a few noise peaks."""
    from ann_solo_amd import decoy_generator as dg
    rng = np.random.default_rng(seed)
    specs = []
    for i in range(n):
        Z = 2 if i % 3 else 3
        c = DC.make_case(rng, int(rng.integers(9, 22)), Z, int(rng.integers(60, 140)), 0.02, 'Da', frac=0.8)
        mass = float(c['masses'].sum()) + R.H2O
        specs.append(FakeSpectrum(f'lib{i:04d}', (mass + Z * R.PROTON) / Z, Z, c['mz'], c['intensity'], None,
                                  c['peptide'], retention_time=float(i)))
    return specs


def _store_sha(path):
    return hashlib.sha256(open(path, 'rb').read()).hexdigest()


def test_decoy_library_end_to_end(tmp_path):
    from ann_solo_amd import decoy_generator as dg
    from ann_solo_amd.config import Config
    from ann_solo_amd.library_store import pack_raw, pack_queries
    from ann_solo_amd.spectral_library import SpectralLibrary
    from ann_solo_amd.spectrum import process_spectra
    specs = _library()
    base = dict(mode='bf', fragment_mz_tolerance=0.02, decoy_tolerance_unit='Da', seed=5, min_mz_range=100.0)
    cfg = Config(device_decoys=True, **base)
    reader = FakeReader(specs, str(tmp_path / 'on' / 'lib.splib'))
    os.makedirs(tmp_path / 'on')
    sl = SpectralLibrary(reader, config=cfg, device='cuda:0')
    assert reader.reads == 1 and sum(len(p.ids) for p in sl.partitions.values()) == 600
    by_id = {s.identifier: s for s in specs}
    n_moved = 0
    for z, part in sl.partitions.items():
        ids = part.ids.tolist()
        targets = ids[1::2]
        assert ids[0::2] == ['DECOY_' + t for t in targets]                       # decoy before its target
        assert targets == reader.spec_info['charge'][z]['id'].tolist()
        assert np.array_equal(part.precursor_mz[0::2], part.precursor_mz[1::2])
        meta = sl.library_meta[z]
        assert [m['is_decoy'] for m in meta] == [True, False] * len(targets)
        assert [m['identifier'] for m in meta] == ids
        # what the rows must hold: process_spectrum of the restatement's raw decoy / of the target with the
        # restatement's charge column
        want = []
        for t, m in zip(targets, meta[0::2]):
            s = by_id[t]
            pep = dg.parse_peptide(s.peptide)
            _, perm = dg.shuffle(pep.sequence, dg.peptide_rng(5, s.peptide, z))
            assert m['peptide'] == str(pep.permuted(perm)) and meta[1]['peptide'] == by_id[targets[0]].peptide
            r = R.decoy_ref(s.mz, s.intensity, pep.masses, perm, pep.nterm, pep.cterm,
                            dg.default_fragment_charge(z), 0.02, 'Da')
            n_moved += int((r['mz'] != s.mz).sum())
            want.append(dg.LibrarySpectrum('d', s.precursor_mz, z, r['mz'], r['intensity'], r['charge'], None, True))
            want.append(dg.LibrarySpectrum('t', s.precursor_mz, z, s.mz, s.intensity, r['ann_z'], None, False))
        ref, valid = process_spectra(pack_raw(want), True, cfg, 'cuda:0')
        got = part.spectra.to('cpu')
        ref = ref.to('cpu')
        assert valid.float().mean() > 0.9
        for a, b in zip(got._tensors()[:4], ref._tensors()[:4]):
            assert torch.equal(a, b)
        assert (got.charge > 0).float().mean() > 0.3
    assert n_moved > 3000
    # queries: noisy copies of targets find their target, not its decoy
    rng = np.random.default_rng(8)
    queries = []
    for j, s in enumerate(specs[::3]):
        keep = rng.random(len(s.mz)) < 0.9
        mz = np.sort((s.mz[keep] + rng.normal(0, 0.003, int(keep.sum()))).astype(np.float32))
        queries.append(FakeSpectrum(f'scan={j}', s.precursor_mz, s.precursor_charge, mz,
                                    s.intensity[keep] * rng.uniform(0.8, 1.25, int(keep.sum())), index=j))
    ssms = sl.search(iter(queries))
    assert len(ssms) == len(queries)
    for s in ssms:
        j = int(s.query_identifier.split('=')[1])
        assert s.library_identifier == specs[3 * j].identifier and s.is_decoy is False
        assert s.sequence == specs[3 * j].peptide
    sl.shutdown()
    # the store came from the cache key of its own; a second engine reads it back without the reader
    on_files = sorted(f for f in os.listdir(tmp_path / 'on') if f.endswith('.spstore'))
    assert len(on_files) == 1
    reader2 = FakeReader(specs, str(tmp_path / 'on' / 'lib.splib'))
    sl2 = SpectralLibrary(reader2, config=cfg, device='cuda:0')
    assert reader2.reads == 0 and [m['is_decoy'] for m in sl2.library_meta[2][:4]] == [True, False, True, False]
    sl2.shutdown()


# name and sha256 of the packed store of _library() under the configuration below, written by the engine of
# the commit before the switch existed (its own package and library build, on an MI355X)
PARENT_STORE_NAME = 'lib_80bb8c1.spstore'
PARENT_STORE_SHA = 'bc40f2583809b8c1166e968e4a78c88b48e8cdee804a09a0684b786254477ba7'


def test_switch_off_leaves_the_store_as_it_was(tmp_path):
    """With device_decoys off nothing is wrapped: the same 300 rows, the same file name and the same
    bytes as the store the engine wrote before the switch existed."""
    from ann_solo_amd.config import Config
    from ann_solo_amd.spectral_library import SpectralLibrary
    specs = _library()
    base = dict(mode='bf', fragment_mz_tolerance=0.02, seed=5, min_mz_range=100.0)
    reader = FakeReader(specs, str(tmp_path / 'lib.splib'))
    sl = SpectralLibrary(reader, config=Config(**base), device='cuda:0')
    assert sl._library_reader is reader
    assert sum(len(p.ids) for p in sl.partitions.values()) == 300
    sl.shutdown()
    files = sorted(f for f in os.listdir(tmp_path) if f.endswith('.spstore'))
    print('store', files, _store_sha(str(tmp_path / files[0])))
    assert files == [PARENT_STORE_NAME]
    assert _store_sha(str(tmp_path / files[0])) == PARENT_STORE_SHA
