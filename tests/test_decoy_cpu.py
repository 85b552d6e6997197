"""Decoy generator, host side: the numpy restatement against the reference's known answer, the
shuffle's properties, the peptide parser, the configuration switch and the reader adapter."""
import argparse
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import decoy_cases as DC     # noqa: E402
import decoy_ref as R        # noqa: E402
from fake_reader import FakeReader, FakeSpectrum   # noqa: E402


def kat():
    return json.load(open(os.path.join(HERE, 'golden', 'decoy_kat.json')))


def test_restatement_reproduces_the_reference_known_answer():
    """Peak order and intensities exactly; m/z within 2e-6 (the restatement measures 9.7e-7 against the
    fixture's 8 printed decimals) -- for the default fragment charge range (Z - 1 = 3) and for 4: the
    fixture does not pin it."""
    from ann_solo_amd import decoy_generator as dg
    k = kat()
    pep = dg.parse_peptide(k['peptide'])
    assert pep.permuted(k['perm']).sequence == dg.parse_peptide(k['decoy_peptide']).sequence
    assert k['unit'] == 'ppm' and k['tolerance'] == 10.0
    for zmax in (dg.default_fragment_charge(k['precursor_charge']), 4):
        r = R.decoy_ref(k['mz'], k['intensity'], pep.masses, k['perm'], 0.0, 0.0, zmax, k['tolerance'], k['unit'])
        want_int = np.asarray(k['decoy_intensity'], np.float32)
        assert np.array_equal(r['intensity'], want_int)
        assert np.array_equal(np.asarray(k['intensity'], np.float32)[r['src']], want_int)
        d = np.abs(r['new_f64'] - np.asarray(k['decoy_mz']))
        print('zmax', zmax, 'max |dmz|', d.max())
        assert d.max() <= 2e-6


def test_shuffle_properties():
    from ann_solo_amd import decoy_generator as dg
    rng = np.random.default_rng(5)
    peptides = []
    for _ in range(200):
        L = int(rng.integers(2, 61))
        text = DC.random_peptide(rng, L, mod_p=0.0)
        peptides.append(text)
        shuffled, perm = dg.shuffle(text, dg.peptide_rng(7, text, 2))
        assert sorted(shuffled) == sorted(text)                                  # composition
        assert sorted(perm) == list(range(L))                                    # a permutation ...
        assert ''.join(text[i] for i in perm) == shuffled                        # ... that makes the string
        for i, a in enumerate(text):
            if i == L - 1 or a in 'KRP':
                assert perm[i] == i and shuffled[i] == a
        again, perm2 = dg.shuffle(text, dg.peptide_rng(7, text, 2))
        assert (again, perm2) == (shuffled, perm)                                # same key, same decoy
    assert any(dg.shuffle(p, dg.peptide_rng(7, p, 2))[0] != dg.shuffle(p, dg.peptide_rng(8, p, 2))[0]
               for p in peptides)
    for fixed in ('KR', 'PK', 'APK', 'KPRPK', 'GK'):                             # nothing to permute
        assert dg.shuffle(fixed, dg.peptide_rng(1, fixed, 2)) == (fixed, list(range(len(fixed))))
    # similarity: the winner is at most 70 % similar wherever any of the draws is
    s, perm = dg.shuffle('ACDEFGHILMNQSTVWYK', dg.peptide_rng(3, 'x', 2))
    assert sum(a == b for a, b in zip(s, 'ACDEFGHILMNQSTVWYK')) < 18


def _stub_batch(calls):
    """Stands in for the device call: the 'decoy' is the raw spectrum with m/z + 1, every peak charge 2
    on the decoy and 1 on the target."""
    from ann_solo_amd.packed import PackedSpectra

    def fn(raw, peptides, tol, unit, seed, device):
        calls.append((raw.n, list(peptides), tol, unit, seed))
        o, mz, it, chg, pmz, pz = raw.numpy()
        decoy = PackedSpectra.from_numpy(o, mz + 1.0, it, np.full(len(mz), 2, np.uint8), pmz, pz, 'cpu',
                                         ['DECOY_' + str(i) for i in raw.identifiers])
        return decoy, [p[::-1] for p in peptides], dict(z=np.ones(len(mz), np.uint8))
    return fn


def test_decoys_do_not_depend_on_the_batch_split():
    """The shuffle is keyed per peptide: the adapter hands the same peptides to the batch call whatever
    its batch size, and the same (seed, peptide, charge) always draws the same permutation."""
    from ann_solo_amd import decoy_generator as dg
    from ann_solo_amd.config import Config
    from ann_solo_amd.library_store import DecoyReader
    rng = np.random.default_rng(2)
    specs = [FakeSpectrum(i, 400.0 + i, 2, np.sort(rng.uniform(100, 900, 12)), rng.random(12), None,
                          DC.random_peptide(rng, 9, mod_p=0.0)) for i in range(7)]
    seen = []
    for batch in (7, 3, 1):
        calls = []
        rd = DecoyReader(FakeReader(specs), Config(device_decoys=True), 'cpu', _stub_batch(calls), batch=batch)
        out = list(rd.read_all_spectra())
        assert [c[0] for c in calls] == [batch] * (7 // batch) + ([7 % batch] if 7 % batch else [])
        seen.append([(s.identifier, s.peptide, s.is_decoy) for s in out])
    assert seen[0] == seen[1] == seen[2]
    a = [dg.shuffle(s.peptide, dg.peptide_rng(11, s.peptide, 2)) for s in specs]
    b = [dg.shuffle(s.peptide, dg.peptide_rng(11, s.peptide, 2)) for s in reversed(specs)][::-1]
    assert a == b


def test_parser():
    from ann_solo_amd import decoy_generator as dg
    p = dg.parse_peptide('AC[Carbamidomethyl]M[+15.994915]S[79.966331]K')
    assert p.sequence == 'ACMSK' and p.deltas == (0.0, 57.021464, 15.994915, 79.966331, 0.0)
    m = p.masses
    assert m[0] == 71.037114 and m[1] == 103.009185 + 57.021464 and m[4] == 128.094963
    assert dg.parse_peptide('N[Deamidated]K').deltas == (0.984016, 0.0)
    with pytest.raises(ValueError):
        dg.parse_peptide('NK/2')
    q = dg.parse_peptide('[Acetyl]-AE[-18.010565]K')
    assert q.nterm == 42.010565 and q.cterm == 0.0 and q.deltas == (0.0, -18.010565, 0.0)
    assert str(q.permuted([1, 0, 2])) == '[+42.010565]-E[-18.010565]AK'
    assert dg.parse_peptide(str(q)) == q
    with pytest.raises(ValueError, match=r'TMT6plex.*lib-17'):
        dg.parse_peptide('AK[TMT6plex]', spectrum='lib-17')
    ext = dg.parse_peptide('AK[TMT6plex]', {'TMT6plex': 229.162932})
    assert ext.deltas == (0.0, 229.162932)
    with pytest.raises(ValueError, match=r"'X'.*lib-3"):
        dg.parse_peptide('AXK', spectrum='lib-3')
    with pytest.raises(ValueError):
        dg.parse_peptide(None, spectrum=4)


# ann_solo_amd.library_store.store_hash at the commit before the decoy options existed
PARENT_KEY_DEFAULT = 'a6906a51207fea94369e332047b8322c6dcd58b0'            # Config(), 'abc', 'peaks'
PARENT_KEY_OPEN = 'f551da15c7130980501b8b8b44a2f07da030e26a'   # open_search(sqrt, 80 peaks), 'abc', 'snapshot'


def test_config_flag_and_store_key():
    from ann_solo_amd.config import Config, add_arguments
    from ann_solo_amd.library_store import store_hash
    p = argparse.ArgumentParser()
    add_arguments(p)
    ns = p.parse_args([])
    assert ns.device_decoys is False and ns.decoy_tolerance_unit == 'ppm'
    ns = p.parse_args(['--device_decoys', '--decoy_tolerance_unit', 'Da', '--ann_seed', '9'])
    cfg = Config.from_reference(ns)
    assert cfg.device_decoys is True and cfg.decoy_tolerance_unit == 'Da' and cfg.seed == 9
    assert Config().device_decoys is False and Config().decoy_tolerance_unit == 'ppm'
    with pytest.raises(ValueError):
        Config(decoy_tolerance_unit='mmu')
    with pytest.raises(SystemExit):
        p.parse_args(['--decoy_tolerance_unit', 'mmu'])
    # the reference's own switch is not ours
    assert Config.from_reference({'add_decoys': True}).device_decoys is False
    # off: the keys of today's stores
    assert store_hash(Config(), 'abc', 'peaks') == PARENT_KEY_DEFAULT
    assert store_hash(Config(decoy_tolerance_unit='Da'), 'abc', 'peaks') == PARENT_KEY_DEFAULT
    open_cfg = dict(scaling='sqrt', max_peaks_used_library=80)
    assert store_hash(Config.open_search(**open_cfg), 'abc', 'snapshot') == PARENT_KEY_OPEN
    # on: a key of its own per option that changes the decoy rows
    keys = {store_hash(Config(device_decoys=True, **kw), 'abc', 'peaks')
            for kw in ({}, {'decoy_tolerance_unit': 'Da'}, {'seed': 5}, {'fragment_mz_tolerance': 0.05})}
    assert len(keys) == 4 and PARENT_KEY_DEFAULT not in keys


def test_index_file_names_change_only_with_the_switch():
    from ann_solo_amd.config import Config
    from ann_solo_amd.spectral_library import SpectralLibrary

    def hashes(cfg):
        sl = SpectralLibrary.__new__(SpectralLibrary)
        sl.config = cfg
        return sl._get_hyperparameter_hash(), sl._get_index_hash()
    h, hi = hashes(Config())
    assert h == hi                                     # the reference's name, as ever
    h2, hi2 = hashes(Config(device_decoys=True))
    assert h2 == h and hi2 != hi
    assert hashes(Config(device_decoys=True, seed=3))[1] != hi2
    assert hashes(Config(index='ivfpq'))[1] != hashes(Config(index='ivfpq', device_decoys=True))[1]


def test_adapter_interleaves_decoys_and_targets():
    from ann_solo_amd.config import Config
    from ann_solo_amd.library_store import DecoyReader
    rng = np.random.default_rng(3)
    specs = []
    for i in range(11):
        z = 2 if i % 3 else 3
        specs.append(FakeSpectrum(f's{i:02d}' if z == 2 else i, 400.0 + 1.37 * i, z,     # ids: text and numbers
                                  np.sort(rng.uniform(100, 900, 15)), rng.random(15), None, f'PEPTIDE{"A" * i}K',
                                  retention_time=float(i)))
    inner = FakeReader(list(reversed(specs)))
    calls = []
    cfg = Config(device_decoys=True, fragment_mz_tolerance=0.05, decoy_tolerance_unit='Da', seed=77)
    rd = DecoyReader(inner, cfg, 'cpu', _stub_batch(calls), batch=4)
    assert rd.is_recreated is False and rd.get_version() == 'null' and rd._filename == inner._filename
    for z, info in inner.spec_info['charge'].items():
        both = rd.spec_info['charge'][z]
        ids = info['id'].tolist()
        assert both['id'].tolist() == [x for i in ids for x in ('DECOY_' + str(i), i)]
        assert both['precursor_mz'].dtype == np.float32
        assert np.array_equal(both['precursor_mz'][0::2], info['precursor_mz'])
        assert np.array_equal(both['precursor_mz'][1::2], info['precursor_mz'])
    out = list(rd.read_all_spectra())
    assert len(out) == 22 and [c[0] for c in calls] == [4, 4, 3]
    assert all(c[2:] == (0.05, 'Da', 77) for c in calls)
    by_id = {s.identifier: s for s in specs}
    for d, t in zip(out[0::2], out[1::2]):
        src = by_id[t.identifier]
        assert d.identifier == 'DECOY_' + str(t.identifier) and d.is_decoy is True and t.is_decoy is False
        assert d.precursor_mz == t.precursor_mz == src.precursor_mz
        assert d.precursor_charge == t.precursor_charge == src.precursor_charge
        assert d.peptide == src.peptide[::-1] and t.peptide == src.peptide and t.retention_time == d.retention_time
        assert np.array_equal(t.mz, src.mz) and np.array_equal(d.mz, src.mz + np.float32(1.0))
        assert np.array_equal(d.intensity, src.intensity)
        assert set(d.charge.tolist()) == {2} and set(t.charge.tolist()) == {1}   # the generator's columns
    # every listed row is delivered, so the packed store can be built from the adapter
    listed = {(z, i) for z, info in rd.spec_info['charge'].items() for i in info['id'].tolist()}
    assert listed == {(s.precursor_charge, s.identifier) for s in out}
    rd.close()
    assert inner.closed
    # a library that holds decoys already
    twice = FakeReader(specs + [FakeSpectrum('DECOY_s01', 500.0, 2, [100.0, 200.0], [1.0, 2.0], None, 'AAK')])
    with pytest.raises(ValueError, match='DECOY_s01'):
        DecoyReader(twice, cfg, 'cpu', _stub_batch([]))


def test_engine_refuses_decoys_for_a_packed_library():
    from ann_solo_amd.config import Config
    from ann_solo_amd.packed import PackedSpectra
    from ann_solo_amd.spectral_library import SpectralLibrary
    pack = PackedSpectra.from_numpy([0, 1], [100.0], [1.0], None, [400.0], [2])
    with pytest.raises(ValueError, match='device_decoys'):
        SpectralLibrary(pack, config=Config(device_decoys=True), device='cpu')


def test_symbol_is_exported():
    from ann_solo_amd import _lib
    assert 'asl_decoy_batch' in _lib.EXPORTS
    assert hasattr(_lib.lib(), 'asl_decoy_batch')
