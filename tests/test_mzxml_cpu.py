"""The mzXML reader's parts that need no GPU: the two value rules the device runs, through their host entries
(``asl_mzxml_duration`` against the Python rule of ``mzxml.duration_minutes``, ``asl_mzxml_pairs`` against numpy's
big-endian views), bit for bit; the same two as a stand-alone program under AddressSanitizer and UBSan
(tests/native/mzxml_check.cpp); the restatement of the dialect (tests/mzxml_ref.py) against hand-written
expectations and on each refusal; the switch."""
import logging
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import mzxml_cases as XC
import mzxml_ref

HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------------------------------------- durations
CONVERTED = ['PT0S', 'PT0.S', 'PT59.999S', 'PT1.5S', 'PT0.25S', 'PT0000123456789.012345S',           # 19 digits, 15 count
             'PT9007199254740991S', 'PT3599.9994S', 'PT007S', 'PT60S', 'PT0.1S', 'PT2345.678901S',
             '12.5', '0', '1e3', '-3.25', '+7', '.5', '5.']                                          # plain numerals
DEFERRED = ['PT1234567890123456789S', 'PT12345678901234567890S',                 # 19 digits (beyond 2^53), 20 digits
            'PT9007199254740993S', 'PT1M2S', 'PT1H', 'P1DT1S', 'PT1H2M3.5S', 'P1Y2M3DT4H5M6S', 'PT2M', 'PT1e3S',
            'PT-1S', 'PT.5S', 'PT5', 'PTS', 'PT', 'P', 'PT 5S', 'pt5s', '-PT5S', '', ' 12.5', 'soon', 'nan', 'inf',
            '1e400', '1_0', 'PT1.5.S', 'PT1S ', 'P5S']


def test_duration_corpus_bit_for_bit():
    """What the device converts equals the Python rule to the bit; what it defers, it defers: it never guesses."""
    from ann_solo_amd import _lib
    from ann_solo_amd.mzxml import duration_minutes
    for text in CONVERTED:
        rc, got = _lib.mzxml_duration(text)
        want, why = duration_minutes(text)
        assert rc == 0 and why is None, text
        assert struct.pack('<d', got) == struct.pack('<d', want), text
    for text in DEFERRED:
        assert _lib.mzxml_duration(text) == (1, None), text
    assert _lib.mzxml_duration('PT59.999S')[1] == 59.999 / 60.0 and _lib.mzxml_duration('PT0.S')[1] == 0.0


def test_the_host_rule_for_what_the_device_defers():
    from ann_solo_amd.mzxml import duration_minutes
    assert duration_minutes('PT1M2S') == (1.0 + 0.0 * 60.0 + 2.0 / 60.0, None)
    assert duration_minutes('PT1H') == (60.0, None)
    assert duration_minutes('P1DT1S') == (1.0 / 60.0, None)                     # the date part is ignored
    assert duration_minutes('PT1H2M3.5S') == (2.0 + 1.0 * 60.0 + 3.5 / 60.0, None)
    assert duration_minutes('PT12345678901234567890S') == (12345678901234567890.0 / 60.0, None)
    assert duration_minutes(' 12.5') == (12.5, None)                            # float() strips blanks
    for bad in ('PT5', 'PTS5', 'P', 'PT', '-PT5S', 'soon', '', 'nan', '1e400', 'PT 5S'):
        v, why = duration_minutes(bad)
        assert v is None and why, bad
    for text in CONVERTED + DEFERRED:                                           # the restatement is the same rule
        v, why = duration_minutes(text)
        if why:
            with pytest.raises(ValueError):
                mzxml_ref.duration_minutes(text)
        else:
            assert struct.pack('<d', mzxml_ref.duration_minutes(text)) == struct.pack('<d', v), text


# ---------------------------------------------------------------------------------------------- pairs
def _pair_cases():
    """(precision, raw big-endian bytes) with the values where a conversion can go wrong."""
    rng = np.random.default_rng(2)
    f64 = np.array([0.0, -0.0, 445.1200256347656, 1e-310, -4.9e-324, 1e-46, 1.401298464324817e-45,   # denormals
                    7.006492321624085e-46, 3.4028234663852886e38, 3.4028235677973366e38,             # just below inf
                    3.4028235677973367e38, -3.5e38, 1e300, np.inf, -np.inf,                          # up to infinity
                    1.0000000596046448, 1.0000001788139343, 16777217.0, 0.1, 1e-38, 1.1754943508222875e-38],
                   np.float64)
    bits64 = np.array([0x7ff8000000000000, 0x7ff8000000000001, 0xfff80000deadbeef, 0x7ff4000000000000,
                       0x7ff0000020000000, 0x7ffc0000a0000000], np.uint64).view(np.float64)         # NaN payloads
    f64 = np.concatenate([f64, bits64, rng.uniform(-1e6, 1e6, 17)])
    f64 = f64[:len(f64) // 2 * 2]
    bits32 = np.array([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x00800000, 0x7f7fffff, 0x7f800000,
                       0xff800000, 0x7fc00000, 0x7fc00001, 0xffc12345, 0x7fa00000, 0x7f800001, 0x3f800000,
                       0x43de8f5c, 0xc2f6e979], np.uint32)
    return [(64, f64.astype('>f8').tobytes()), (32, bits32.astype('>u4').tobytes()),
            (64, b''), (32, b''), (32, rng.uniform(100, 2000, 2 * 301).astype('>f4').tobytes())]


def _numpy_pairs(precision, raw):
    with np.errstate(over='ignore', invalid='ignore'):
        v = np.frombuffer(raw, '>f8' if precision == 64 else '>f4').astype(np.float32)
    return v[0::2].copy(), v[1::2].copy()


def test_pairs_against_numpy_as_bytes():
    from ann_solo_amd import _lib
    for precision, raw in _pair_cases():
        n = len(raw) // (precision // 4)
        mz, it = _lib.mzxml_pairs(raw, n, precision)
        want_mz, want_it = _numpy_pairs(precision, raw)
        assert mz.dtype == np.float32 and mz.tobytes() == want_mz.tobytes(), precision
        assert it.tobytes() == want_it.tobytes(), precision
    mz, it = _lib.mzxml_pairs(np.array([1e39, -1e39, 3.4028234663852886e38, 1e-50], '>f8').tobytes(), 2, 64)
    assert mz.tolist() == [np.inf, np.float32(3.4028234663852886e38)] and it.tolist() == [-np.inf, 0.0]
    with pytest.raises(ValueError):
        _lib.mzxml_pairs(b'\0' * 8, 1, 16)
    with pytest.raises(ValueError):
        _lib.mzxml_pairs(b'\0' * 9, 1, 32)


# ---------------------------------------------------------------------------------------------- sanitizer program
def test_value_rules_under_the_sanitizers(tmp_path):
    """The same durations and pairs through the stand-alone program: no Python process loads sanitized code."""
    from ann_solo_amd.mzxml import duration_minutes
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = tmp_path / 'mzxml_check'
    src = os.path.join(HERE, 'native', 'mzxml_check.cpp')
    inc = os.path.join(HERE, '..', 'ann_solo_amd', 'csrc')
    base = [cxx, '-std=c++17', '-O1', '-g', '-I', inc, src, '-o', str(exe)]
    built = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True,
                           text=True)
    assert built.returncode == 0, built.stderr       # (a toolchain that cannot link a sanitized program fails here)
    recs = []
    for text in CONVERTED:
        recs.append(struct.pack('<BBI', 0, 0, len(text)) + text.encode() + struct.pack('<d', duration_minutes(text)[0]))
    for text in DEFERRED:
        recs.append(struct.pack('<BBI', 0, 1, len(text)) + text.encode() + bytes(8))
    for precision, raw in _pair_cases():
        mz, it = _numpy_pairs(precision, raw)
        recs.append(struct.pack('<BBI', 1, precision, len(mz)) + raw + mz.tobytes() + it.tobytes())
    corpus = tmp_path / 'corpus.bin'
    corpus.write_bytes(b''.join(recs))
    run = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert f'{len(recs)} records, 0 mismatches' in run.stdout


# ---------------------------------------------------------------------------------------------- the restatement
MZ, IT = np.array([100.5, 200.25, 300.125]), np.array([1.0, 2.0, 3.0])


def test_restatement_reads_the_named_cases(caplog):
    ms3 = XC.scan(4, MZ, IT, level=3, pad='        ')
    kids = [XC.scan(2, MZ, IT, charge=3, rt='PT90S', pmz='444.5', f64=True, z=True, pad='      '),
            XC.scan(3, MZ[::-1], IT, charge=None, rt='PT1M30S', pmz=' 445.5 ', pad='      ', children=[ms3],
                    order='pairOrder')]
    scans = [XC.scan(1, MZ, IT, level=1, children=kids),
             XC.scan(' 7 ', MZ, IT, rt='2.5', byte_order=None, order=None, compression=''),    # bare <peaks precision>
             XC.scan('seven', MZ, IT),
             XC.scan(9, (), (), peaks_xml=XC.peaks_tag(self_closing=True)),
             XC.scan(10, MZ, IT, level=None)]
    with caplog.at_level(logging.WARNING):
        got = mzxml_ref.read_mzxml(XC.document(scans))
    assert [(s.index, s.identifier, s.precursor_charge, s.nested) for s in got] == \
        [(1, '2', 3, True), (2, '3', None, True), (4, '7', 2, False), (6, '9', 2, False)]
    assert (got[0].precursor_mz, got[0].retention_time) == (444.5, 1.5)
    assert (got[1].precursor_mz, got[1].retention_time) == (445.5, 1.5) and got[2].retention_time == 2.5
    assert got[0].mz.dtype == np.float64 and got[1].mz.dtype == np.float32
    assert np.array_equal(got[0].mz, MZ) and np.array_equal(got[0].intensity, IT)
    assert np.array_equal(got[1].mz, MZ[::-1].astype(np.float32))                # (pack_raw sorts)
    assert len(got[3].mz) == 0 and len(got[3].intensity) == 0
    assert sum('failed to read scan' in r.message for r in caplog.records) == 1
    flat = mzxml_ref.read_mzxml(XC.document(scans, newlines=False, index=False))
    assert [s.identifier for s in flat] == ['2', '3', '7', '9']
    assert mzxml_ref.read_mzxml(b'') == [] and mzxml_ref.read_mzxml(XC.document([])) == []


REFUSALS = [
    (dict(rt=None), 'scan 1: no retentionTime'),
    (dict(rt='PT5'), "scan 1: retentionTime 'PT5' is not a duration"),
    (dict(rt='soon'), "scan 1: retentionTime 'soon' is not a number"),
    (dict(rt='1e400'), 'scan 1: non-finite retentionTime'),
    (dict(pmz=None), 'scan 1: no <precursorMz>'),
    (dict(pmz='heavy'), "scan 1: precursor m/z 'heavy' is not a number"),
    (dict(pmz=''), 'scan 1: precursor m/z'),
    (dict(charge='2+'), 'scan 1: precursorCharge'),
    (dict(charge=0), 'scan 1: precursorCharge'),
    (dict(charge=256), 'scan 1: precursorCharge'),
    (dict(count=4), 'scan 1: 24 bytes, peaksCount promises 32'),
    (dict(count=2), 'scan 1: 24 bytes, peaksCount promises 16'),
    (dict(count='many'), 'scan 1: peaksCount'),
    (dict(count=False), 'scan 1: peaksCount None'),
    (dict(level='two'), 'scan 1: msLevel'),
    (dict(precision='16'), 'scan 1: a missing or unsupported precision'),
    (dict(precision=''), 'scan 1: a missing or unsupported precision'),
    (dict(byte_order='little'), 'scan 1: byteOrder'),
    (dict(order_value='int-m/z'), 'scan 1: a contentType or pairOrder'),
    (dict(order='pairOrder', order_value='intensity'), 'scan 1: a contentType or pairOrder'),
    (dict(compression='gzip'), 'scan 1: compressionType'),
    (dict(peaks_xml=XC.peaks_tag(MZ, IT) + XC.peaks_tag(MZ, IT)), 'scan 1: more than one <peaks>'),
    (dict(peaks_xml=''), 'scan 1: no <peaks>'),
    (dict(content='AAA*'), 'scan 1: not base64'),
    (dict(content=XC.encode(MZ, IT)[:-1]), 'scan 1: not base64'),
    (dict(z=True, content=XC.encode(MZ, IT)), 'scan 1: Error -3'),
    (dict(inside='<!-- late -->'), 'scan 1: a comment'),
    (dict(inside='<userParam><![CDATA[x]]></userParam>'), 'scan 1: a comment'),
    (dict(inside='<peaks precision="32"></peaks>', children=[XC.scan(5, MZ, IT, level=3)]), 'a <peaks> outside'),
]


def _refused(change):
    return XC.document([XC.scan(1, MZ, IT), XC.scan(2, MZ, IT, **change), XC.scan(3, MZ, IT)])


@pytest.mark.parametrize('change, text', REFUSALS, ids=[str(k) for k in range(len(REFUSALS))])
def test_restatement_refuses(change, text):
    with pytest.raises(ValueError, match=text):
        mzxml_ref.read_mzxml(_refused(change))


def test_restatement_capacity_and_a_missing_num():
    big = np.arange(4097) + 100.0
    with pytest.raises(OverflowError, match='scan 0'):
        mzxml_ref.read_mzxml(XC.document([XC.scan(1, big, big)]))
    data = XC.document([XC.scan(1, MZ, IT)]).replace(b'num="1"', b'')
    with pytest.raises(ValueError, match='scan 0: no num'):
        mzxml_ref.read_mzxml(data)


# ---------------------------------------------------------------------------------------------- the switch
def test_switch_and_flag():
    from ann_solo_amd import config
    assert config.Config().device_mzxml is False and config.Config(device_mzxml=1).device_mzxml is True
    src = open(os.path.join(HERE, '..', 'ann_solo_amd', 'config.py')).read()
    assert "'--device_mzxml'" in src and 'mzXML is read as before' not in src


def test_far_stream_is_what_it_says():
    stream, raw, mz, it = XC.far_stream()
    assert len(raw) == 65536 and raw[-8:] == raw[32760:32768] and np.all(np.diff(mz) >= 0)
    # the last block is one match of length 8 at the largest distance DEFLATE has
    from ann_solo_amd import _lib
    import base64
    assert _lib.mzml_inflate(base64.b64encode(stream), True, 65536) == (0, raw)  # the core takes a 64 KiB window
    assert _lib.mzml_inflate(base64.b64encode(stream), True, 65535)[0] == 12
