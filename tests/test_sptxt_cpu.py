"""CPU side of the .sptxt library reader (``Config.device_library``): the annotation rule the kernels call
(``asl_sptxt_fragment_charge``, run on the host) against the restatement's, the ProForma function and the
restatement itself against literals, the ABI's checks that need no device, and the switch."""
import argparse

import numpy as np
import pytest

import sptxt_cases as SC
import sptxt_ref


# ---------------------------------------------------------------------------------------------- annotations
def test_fragment_charge_every_first_character_and_tail():
    from ann_solo_amd import _lib
    cases = SC.annotation_cases()
    got = [_lib.sptxt_fragment_charge(a) for a in cases]
    assert got == [sptxt_ref.fragment_charge(a) for a in cases]
    assert 0 in got and 1 in got and 2 in got and 3 in got and 255 in got


def test_fragment_charge_literals():
    from ann_solo_amd import _lib
    f = _lib.sptxt_fragment_charge
    assert [f(a) for a in ('b5/0.01', 'y7^2/0.02', 'y3-18^2/0.01,b4/0.3', '?', 'p^3/0.0', 'a2', 'IKD/0.0', '')] == \
        [1, 2, 2, 0, 3, 1, 0, 0]
    assert [f(a) for a in ('y', 'y^', 'y^x', 'y^0', 'y^255', 'y^256', 'y^99999999999', 'b3/0.1^2', 'b3^2^3', 'Y5^2',
                           ' b5^2', 'y5/0.1,b3^2/0.2')] == [1, 1, 1, 0, 255, 255, 255, 1, 2, 0, 0, 1]
    assert f(b'y5^2\xff') == 2 and f(b'\xff') == 0
    assert _lib.lib().asl_sptxt_fragment_charge(None, 0) == 0 and _lib.lib().asl_sptxt_fragment_charge(b'y^2', -1) == 0
    assert _lib.lib().asl_sptxt_fragment_charge(b'y^23', 3) == 2          # the length rules


def test_fragment_charge_random_annotations():
    from ann_solo_amd import _lib
    cases = SC.random_annotations(20000, seed=11)
    got = np.array([_lib.sptxt_fragment_charge(a) for a in cases])
    assert got.tolist() == [sptxt_ref.fragment_charge(a) for a in cases]
    assert (got == 0).sum() > 1000 and (got == 1).sum() > 1000 and (got > 1).sum() > 1000


# ---------------------------------------------------------------------------------------------- ProForma
@pytest.mark.parametrize('peptide, mods, want', [
    ('AAAK', None, 'AAAK'),
    ('AAAK', '0', 'AAAK'),
    ('ACDEK', '1/1,C,Carbamidomethyl', 'AC[Carbamidomethyl]DEK'),
    ('MACMK', '3/0,M,Oxidation/2,C,Carbamidomethyl/3,M,Oxidation', 'M[Oxidation]AC[Carbamidomethyl]M[Oxidation]K'),
    ('AAAK', '1/-1,A,Acetyl', '[Acetyl]AAAK'),
    ('AAAK', '2/-1,A,Acetyl/0,A,Oxidation', '[Acetyl]A[Oxidation]AAK'),
    ('AAAK', '1/3,K,Phospho', 'AAAK[Phospho]'),
    ('AAAK', '2/1,A,X/1,A,Y', 'AA[X][Y]AK'),
    ('AAAK', '', 'AAAK'),
])
def test_proforma_literals(peptide, mods, want):
    from ann_solo_amd import sptxt
    assert sptxt.proforma(peptide, mods) == want
    assert sptxt_ref.proforma(peptide, mods) == want


@pytest.mark.parametrize('peptide, mods', [
    ('AAa', None), ('n[43]AAAK', None), ('A[Oxidation]K', '0'), ('', None), ('AA-K', None), ('AAK2', None),
    ('AAAK', '1/4,K,Phospho'), ('AAAK', '1/-2,A,Acetyl'), ('AAAK', '1/1,A'), ('AAAK', '1/1,A,B,C'),
    ('AAAK', '1/x,A,Acetyl'), ('AAAK', '2/2,A,X/1,A,Y'), ('AAAK', '1/1_0,A,X'),
])
def test_proforma_refusals(peptide, mods):
    from ann_solo_amd import sptxt
    with pytest.raises(ValueError):
        sptxt.proforma(peptide, mods)
    with pytest.raises(ValueError):
        sptxt_ref.proforma(peptide, mods)


# ---------------------------------------------------------------------------------------------- the restatement
TWO_RECORDS = (b'### preamble, FullName: x\r\n'
               b'Name: ACDEK/2\r\n'
               b'MW: 1000.5\r\n'
               b'PrecursorMZ: 500.25\r\n'
               b'Comment: Mods=1/1,C,Carbamidomethyl Parent=501.000 Spec=x\r\n'
               b'Num Peaks: 3\r\n'
               b'300.5\t20\tb3^2/0.01\t1/2\r\n'
               b'\r\n'
               b'100.25\t10.5\ty1/0.0 # a tail\r\n'
               b'200.125\t30\t?\r\n'
               b'name: DECOY_0 MAAK/3/x\n'
               b'Comment: Parent= 250.5 mods=1/-1,M,Acetyl\n'
               b'NUMPEAKS: 1\n'
               b' 7 \t 8 \t\tq')


def test_restatement_against_literals():
    a, b = sptxt_ref.read_sptxt(TWO_RECORDS)
    assert (a.identifier, a.precursor_mz, a.precursor_charge, a.peptide, a.is_decoy) == \
        ('1', 500.25, 2, 'AC[Carbamidomethyl]DEK', False)
    assert a.mz.tolist() == [300.5, 100.25, 200.125] and a.intensity.tolist() == [20.0, 10.5, 30.0]   # file order
    assert [0 if x is None else x.charge for x in a.annotation] == [2, 1, 0]
    assert (b.identifier, b.precursor_mz, b.precursor_charge, b.peptide, b.is_decoy) == \
        ('2', 250.5, 3, '[Acetyl]MAAK', True)
    assert b.mz.tolist() == [7.0] and b.intensity.tolist() == [8.0] and b.annotation == [None]
    assert a.mz.dtype == np.float64
    from ann_solo_amd.library_store import pack_raw
    raw = pack_raw([a, b])
    assert raw.mz.tolist() == [100.25, 200.125, 300.5, 7.0] and raw.charge.tolist() == [1, 0, 2, 0]   # charges travel


@pytest.mark.parametrize('text, where', SC.REFUSALS)
def test_restatement_refusals(text, where):
    with pytest.raises(ValueError, match=where + ':'):
        sptxt_ref.read_sptxt(text)


# ---------------------------------------------------------------------------------------------- ABI, switch
def test_chunk_of_two_gib_is_refused_before_any_pointer_is_touched():
    from ann_solo_amd import _lib
    counts = np.zeros(16, np.int64)
    rc = _lib.lib().asl_sptxt_measure(0xdead0000, 1 << 31, 1, counts.ctypes.data_as(_lib.c_i64p))
    assert rc == _lib.ERR_CAPACITY
    assert _lib.lib().asl_sptxt_measure(None, -1, 1, counts.ctypes.data_as(_lib.c_i64p)) == _lib.ERR_INVALID
    assert _lib.lib().asl_sptxt_measure(None, 0, 2, counts.ctypes.data_as(_lib.c_i64p)) == _lib.ERR_INVALID
    assert _lib.lib().asl_sptxt_measure(None, 0, 1, counts.ctypes.data_as(_lib.c_i64p)) == 0      # n == 0 is legal
    assert counts[1] == 0 and counts[7] == -1


def test_constants_match_the_header():
    import os
    import re
    from ann_solo_amd import _lib, sptxt
    with open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'annsolo_mi.h')) as f:
        head = f.read()
    defs = dict(re.findall(r'#define (ASL_SPTXT_[A-Z_]+) (-?\d+)', head))
    names = ['N_LINES', 'N_RECORDS', 'N_PEAKS', 'N_DEFERRED', 'CONSUMED', 'CONSUMED_LINES', 'ERR_KIND', 'ERR_LINE',
             'OPEN']
    assert [int(defs['ASL_SPTXT_' + n]) for n in names] == list(range(9)) and int(defs['ASL_SPTXT_COUNTS']) == 9
    assert [int(defs['ASL_SPTXT_DEST_' + n]) for n in ('MZ', 'INTENSITY', 'PRECURSOR', 'NONE')] == list(range(4))
    assert int(defs['ASL_SPTXT_INFO']) == sptxt._INFO
    kinds = ['SECOND_NAME', 'SECOND_NUMPEAKS', 'NUMPEAKS', 'FEW_FIELDS', 'PRECURSOR', 'STRAY_KEY']
    assert [int(defs['ASL_SPTXT_ERR_' + n]) for n in kinds] == sorted(sptxt._ERR_TEXT)
    for name in ('asl_sptxt_measure', 'asl_sptxt_fill', 'asl_sptxt_fragment_charge', 'asl_mgf_sort_charged'):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)


def test_config_switch_and_hashes():
    from ann_solo_amd import library_store as ls
    from ann_solo_amd.config import Config, add_arguments
    from ann_solo_amd.spectral_library import SpectralLibrary
    assert Config().device_library is False
    p = argparse.ArgumentParser()
    add_arguments(p)
    assert p.parse_args([]).device_library is False
    cfg = Config.from_reference(p.parse_args(['--device_library']))
    assert cfg.device_library is True and Config.from_reference({'device_library': 1}).device_library is True

    def hashes(**kw):
        sl = SpectralLibrary.__new__(SpectralLibrary)
        sl.config = Config(**kw)
        return sl._get_index_hash(), ls.store_hash(sl.config, sl._get_hyperparameter_hash(), 'peaks')
    # off: the literals of the commit before the switch existed
    assert hashes() == ('8d8eea45d2dab04edf9e79da76bbd78d8a8c956b', '149f57dd8c973b59093f039f9f5680fe6c052498')
    assert hashes(index='ivfpq') == ('9e7f74f579c1efb16939239fbbde1bc1cb282b8a',
                                     '149f57dd8c973b59093f039f9f5680fe6c052498')
    assert hashes(device_decoys=True) == ('2a9f75eb76661678771c81f049202057c35de4bf',
                                          '3cc781bb444c2ad448ede7e30b45680c2611e556')
    # on: the index name stays (the same rows under the same identifiers), the store's key moves
    on = hashes(device_library=True)
    assert on[0] == '8d8eea45d2dab04edf9e79da76bbd78d8a8c956b' and on[1] != '149f57dd8c973b59093f039f9f5680fe6c052498'


def test_snapshot_alignment_with_the_switch_is_an_error(tmp_path):
    from ann_solo_amd.config import Config
    from ann_solo_amd.spectral_library import SpectralLibrary
    path = tmp_path / 'lib.SpTxt'
    path.write_bytes(TWO_RECORDS)
    with pytest.raises(ValueError, match='annotation_alignment'):
        SpectralLibrary(str(path), config=Config(device_library=True, mode='bf'), annotation_alignment='snapshot')
