"""CPU side of the MGF reader (``Config.device_mgf``): the Python restatement of the dialect against literals,
the numeral converter (``asl_mgf_number``, the function the kernels call, run on the host) against ``float()``
bit for bit and its deferred set against a second statement of the rule, the ABI's checks that need no device,
and the switch."""
import argparse
import ctypes as C
import logging
import struct

import numpy as np
import pytest

import mgf_cases as MC
import mgf_ref


def _bits(x: float) -> int:
    return struct.unpack('<Q', struct.pack('<d', x))[0]


# ---------------------------------------------------------------------------------------------- the restatement
def test_restatement_against_literals(caplog):
    with caplog.at_level(logging.WARNING):
        got = mgf_ref.read_mgf(MC.HAND_WRITTEN)
    assert any('not closed' in r.message for r in caplog.records)        # the fourth block is dropped
    assert [s.identifier for s in got] == ['first = one', '17', '']
    assert [s.index for s in got] == [1, 2, 3]
    assert [s.precursor_mz for s in got] == [500.25, 600.75, 500.0]       # first token; last duplicate; .5e3
    assert [s.precursor_charge for s in got] == [2, 4, 1]                 # header default; last duplicate; list
    assert [s.retention_time for s in got] == [12.5, None, None]
    assert got[0].mz.tolist() == [100.5, 200.25, 300.125] and got[0].intensity.tolist() == [10.0, 20.0, 30.0]
    assert got[1].mz.tolist() == [150.5, 50.25] and got[1].intensity.tolist() == [1.5, 2.5]      # file order, CRLF
    assert got[2].mz.tolist() == [7.0] and got[2].intensity.tolist() == [8.0]
    assert got[0].mz.dtype == np.float64


def test_restatement_charge_none_and_lists():
    block = b'BEGIN IONS\nTITLE=a\nPEPMASS=1\n%s1 2\nEND IONS\n'
    z = lambda line: mgf_ref.read_mgf(block % line)[0].precursor_charge
    assert z(b'') is None
    assert [z(b'CHARGE=%s\n' % v) for v in (b'2+', b'2', b'+2', b'3+', b'2,3', b'2+ and 3+', b'4+,5+', b' 255 ')] == \
        [2, 2, 2, 3, 2, 2, 4, 255]
    for bad in (b'0', b'256', b'2-', b'-2', b'', b'two', b'+2+', b'2 3'):
        with pytest.raises(ValueError, match='spectrum 1'):
            z(b'CHARGE=%s\n' % bad)


@pytest.mark.parametrize('text, where', [
    (b'BEGIN IONS\nTITLE=a\nPEPMASS=1\n5\nEND IONS\n', 'line 4'),
    (b'x\nBEGIN IONS\nTITLE=a\nBEGIN IONS\n', 'line 4'),
    (b'BEGIN IONS\nTITLE=a\nPEPMASS=1\n1 2\n3 x\nEND IONS\n', 'line 5'),
    (b'BEGIN IONS\nTITLE=a\nPEPMASS=1\nnan 2\nEND IONS\n', 'line 4'),
    (b'BEGIN IONS\nTITLE=a\nPEPMASS=1\n1 1e999\nEND IONS\n', 'line 4'),
    (b'BEGIN IONS\nTITLE=a\n1 2\nEND IONS\n', 'spectrum 1'),
    (b'BEGIN IONS\nTITLE=a\nPEPMASS=1\nEND IONS\nBEGIN IONS\nPEPMASS=1\n1 2\nEND IONS\n', 'spectrum 2'),
    (b'BEGIN IONS\nTITLE=a\nPEPMASS=inf\n1 2\nEND IONS\n', 'spectrum 1'),
    (b'BEGIN IONS\nTITLE=a\nPEPMASS=\n1 2\nEND IONS\n', 'spectrum 1'),
    (b'BEGIN IONS\nTITLE=a\nPEPMASS=1\nCHARGE=300\n1 2\nEND IONS\n', 'spectrum 1'),
])
def test_restatement_deviations(text, where):
    with pytest.raises(ValueError, match=where + ':'):
        mgf_ref.read_mgf(text)


# ---------------------------------------------------------------------------------------------- numerals
def _check(tokens):
    from ann_solo_amd import _lib
    n_converted = 0
    for tok in tokens:
        rc, value = _lib.mgf_number(tok)
        assert rc == int(MC.needs_host(tok)), tok
        if rc == 0:
            assert _bits(value) == _bits(float(tok)), tok
            n_converted += 1
    return n_converted


def test_number_random_numerals_match_float_bit_for_bit():
    tokens = MC.random_numerals(100000, seed=20)
    n = _check(tokens)
    assert 0.5 * len(tokens) < n < len(tokens)           # neither everything nor nothing is deferred


def test_number_edges():
    n = _check(MC.EDGES)
    assert 15 <= n < len(MC.EDGES) - 15                  # the list has both kinds in number
    from ann_solo_amd import _lib
    assert _lib.mgf_number(str(2 ** 53 - 1)) == (0, float(2 ** 53 - 1)) and _lib.mgf_number(str(2 ** 53))[0] == 1
    assert _lib.mgf_number('1e22') == (0, 1e22) and _lib.mgf_number('1e23')[0] == 1
    assert _lib.mgf_number('1e-22') == (0, 1e-22) and _lib.mgf_number('1e-23')[0] == 1
    assert _bits(_lib.mgf_number('-0')[1]) == _bits(-0.0) == _bits(_lib.mgf_number('-0.0e400')[1])
    assert _lib.mgf_number('0' * 400 + '1.5') == (0, 1.5)
    assert _lib.mgf_number('1234567890123456789')[0] == 1 and _lib.mgf_number('12345678901234567890')[0] == 1
    assert _lib.mgf_number('999999999999999') == (0, 999999999999999.0)
    assert _lib.mgf_number('9' * 16)[0] == 1             # above 2^53
    for tok in MC.REFUSED + MC.NON_FINITE:               # what float() refuses or maps to inf / nan is never guessed
        assert _lib.mgf_number(tok)[0] == 1, tok


def test_needs_host_is_a_rule_of_its_own():
    assert [MC.needs_host(t) for t in (b'1.5', b'-0.0e400', b'.5', b'5.', b'1e22', b'9007199254740991')] == [False] * 6
    assert [MC.needs_host(t) for t in (b'1e23', b'9007199254740992', b'nan', b'1_0', b'', b'1 ')] == [True] * 6


def test_number_null_and_embedded_bytes():
    from ann_solo_amd import _lib
    L = _lib.lib()
    out = C.c_double(7.0)
    assert L.asl_mgf_number(None, 0, C.byref(out)) == 1 and out.value == 7.0
    assert L.asl_mgf_number(b'12', -1, C.byref(out)) == 1
    assert L.asl_mgf_number(b'12\x003', 4, C.byref(out)) == 1 and out.value == 7.0     # a NUL is a stray byte
    assert L.asl_mgf_number(b'123', 2, C.byref(out)) == 0 and out.value == 12.0        # the length rules


# ---------------------------------------------------------------------------------------------- ABI, switch
def test_chunk_of_two_gib_is_refused_before_any_pointer_is_touched():
    from ann_solo_amd import _lib
    counts = np.zeros(16, np.int64)
    rc = _lib.lib().asl_mgf_measure(0xdead0000, 1 << 31, 1, counts.ctypes.data_as(_lib.c_i64p))
    assert rc == _lib.ERR_CAPACITY
    with pytest.raises(_lib.AnnSoloMiError) as e:
        _lib.check(rc)
    assert e.value.code == _lib.ERR_CAPACITY and '2^31' in str(e.value)
    assert _lib.lib().asl_mgf_measure(None, -1, 1, counts.ctypes.data_as(_lib.c_i64p)) == _lib.ERR_INVALID
    assert _lib.lib().asl_mgf_measure(None, 0, 2, counts.ctypes.data_as(_lib.c_i64p)) == _lib.ERR_INVALID


def test_constants_match_the_header():
    import os
    import re
    from ann_solo_amd import _lib, mgf
    with open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'annsolo_mi.h')) as f:
        head = f.read()
    defs = dict(re.findall(r'#define (ASL_MGF_[A-Z_]+) (-?\d+)', head))
    assert int(defs['ASL_MGF_TILE']) == _lib.MGF_TILE == mgf.SCAN_TILE
    assert int(defs['ASL_MGF_MAX_PEAKS']) == _lib.MGF_MAX_PEAKS == mgf.MAX_PEAKS == 4096
    assert int(defs['ASL_MGF_MAX_LINE']) == _lib.MGF_MAX_LINE
    names = ['N_LINES', 'N_SPECTRA', 'N_PEAKS', 'N_DEFERRED', 'CONSUMED', 'CONSUMED_LINES', 'ERR_KIND', 'ERR_LINE',
             'OPEN']
    assert [int(defs['ASL_MGF_' + n]) for n in names] == list(range(9)) and int(defs['ASL_MGF_COUNTS']) == 9
    assert [int(defs['ASL_MGF_DEST_' + n]) for n in ('MZ', 'INTENSITY', 'PEPMASS', 'RT', 'NONE')] == list(range(5))
    for name in ('asl_mgf_measure', 'asl_mgf_fill', 'asl_mgf_sort', 'asl_mgf_number'):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)


def test_config_switch():
    from ann_solo_amd.config import Config, add_arguments
    assert Config().device_mgf is False
    p = argparse.ArgumentParser()
    add_arguments(p)
    assert p.parse_args([]).device_mgf is False
    ns = p.parse_args(['--device_mgf'])
    cfg = Config.from_reference(ns)
    assert cfg.device_mgf is True
    assert Config.from_reference(cfg) is cfg and Config.from_reference(cfg, fdr=0.05).device_mgf is True
    assert Config.from_reference({'device_mgf': 1}).device_mgf is True
    # the switch only produces search_packed's input: it combines with every other option
    assert Config(device_mgf=True, num_gpus=2).device_mgf and Config(device_mgf=True, device_fdr=True).device_mgf


def test_header_charge_of_the_driver_is_the_restatement():
    from ann_solo_amd import mgf
    for v in (b'2+', b'2', b'+2', b'2+ and 3+', b'2,3', b'4+,5+', b' 255 ', b'0', b'256', b'2-', b'-2', b'', b'two',
              b'+2+', b'2 3', b'2and3'):
        try:
            want = mgf_ref.parse_charge(v, 'x')
        except ValueError:
            want = -1
        assert mgf._header_charge(v) == want, v
