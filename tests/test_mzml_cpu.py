"""The mzML reader's parts that need no GPU: the decoder core of csrc/inflate.hpp through its host entry
(``_lib.mzml_inflate`` = ``asl_mzml_inflate``) against Python's ``base64`` and ``zlib``; the same core as a
stand-alone program under AddressSanitizer and UBSan (tests/native/inflate_check.cpp); the restatement of the dialect
(tests/mzml_ref.py) against hand-written expectations; the switch."""
import base64
import logging
import os
import shutil
import subprocess

import numpy as np
import pytest

import mzml_cases as MC
import mzml_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CAP = 4096 * 8


def inflate(stream: bytes, cap=CAP, use_zlib=True):
    from ann_solo_amd import _lib
    return _lib.mzml_inflate(base64.b64encode(stream), use_zlib, cap)


# ---------------------------------------------------------------------------------------------- inflate
@pytest.mark.parametrize('n', [0, 1, 2, 3, CAP, CAP + 1])
def test_stream_lengths(n):
    raw = np.random.default_rng(n).integers(0, 200, n, dtype=np.uint8).tobytes()
    for level in (0, 6):
        rc, out = inflate(MC.deflate(raw, level))
        if n > CAP:
            assert rc == 12 and out is None          # the sink overflows: an error, nothing written beyond it
        else:
            assert rc == 0 and out == raw


def test_levels_strategies_and_block_structures():
    seen = set()
    for name, stream, raw in MC.streams():
        rc, out = inflate(stream, len(raw))
        assert rc == 0 and out == raw, name
        assert inflate(stream, len(raw) - 1)[0] == 12, name
        seen.add((stream[2] >> 1) & 3)               # the first block's type
    assert seen == {0, 1, 2}                         # stored, fixed and dynamic blocks were all decoded


def test_full_flush_holds_empty_stored_blocks():
    stream = dict((n, s) for n, s, _ in MC.streams())['full-flush']
    assert stream.count(b'\x00\x00\xff\xff') >= 2


def test_far_and_overlapping_matches():
    stream, raw = MC.far_stream()                                # one match at distance 32 760
    assert len(raw) == CAP and raw[:8] == raw[-8:] and len(stream) < CAP + 64
    assert inflate(stream) == (0, raw)
    assert len(MC.deflate(dict(MC.named_arrays())['constant'], 9)) < 200         # runs of length 258 at distance 8


@pytest.mark.parametrize('which', [0, 1])
def test_every_truncation_and_bit_flip(which):
    """Our verdict is zlib.decompress's, error <=> exception, in every case; the bytes wherever both succeed."""
    name, stream = MC.small_streams()[which]
    assert (stream[2] >> 1) & 3 == (0, 2)[which], name           # a stored, a dynamic stream
    n = n_ok = 0
    for m in MC.mutations(stream):
        want = MC.python_verdict(m)
        rc, out = inflate(m, 4096)
        assert (rc != 0) == (want is None), (name, n, rc)
        if want is not None:
            assert out == want, (name, n)
            n_ok += 1
        n += 1
    assert n == 9 * len(stream) and 0 < n_ok < n


def test_base64():
    from ann_solo_amd import _lib
    dec = lambda s: _lib.mzml_inflate(s, False, 64)
    assert dec(b'') == (0, b'')
    assert dec(b'QQ==') == (0, b'A') and dec(b'QUI=') == (0, b'AB') and dec(b'QUJD') == (0, b'ABC')
    assert dec(b' QU\tJD\r\nQUJD \n') == (0, b'ABCABC')           # blanks inside
    assert dec(b'QU*D')[0] == 1 and dec(b'QUJD\x00')[0] == 1      # a stray byte
    assert dec(b'QUJ')[0] == 2 and dec(b'QUJDQ')[0] == 2          # a bad length
    for bad in (b'Q=JD', b'QU=D', b'QUI=QUJD', b'====', b'QUJD===='):
        assert dec(bad)[0] == 3, bad                              # padding anywhere but at the end
    whole = bytes(range(256)) * 3
    assert dec(base64.b64encode(whole))[0] == 12 and _lib.mzml_inflate(base64.b64encode(whole), False, 768) == \
        (0, whole)


# ---------------------------------------------------------------------------------------------- sanitizer program
def test_decoder_core_under_the_sanitizers(tmp_path):
    """The same truncations and flips, and the named streams, through the stand-alone program."""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = tmp_path / 'inflate_check'
    src = os.path.join(HERE, 'native', 'inflate_check.cpp')
    inc = os.path.join(HERE, '..', 'ann_solo_amd', 'csrc')
    base = [cxx, '-std=c++17', '-O1', '-g', '-I', inc, src, '-o', str(exe)]
    built = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True,
                           text=True)
    assert built.returncode == 0, built.stderr       # (a toolchain that cannot link a sanitized program fails here)
    recs = []
    for _, stream, raw in MC.streams():
        recs.append(MC.corpus_record(base64.b64encode(stream), True, len(raw), raw))
        recs.append(MC.corpus_record(base64.b64encode(stream), True, len(raw) - 1, None))
    for _, stream in MC.small_streams():
        for m in MC.mutations(stream):
            recs.append(MC.corpus_record(base64.b64encode(m), True, 4096, MC.python_verdict(m)))
    for text, want in [(b'', b''), (b'QQ==', b'A'), (b'QUI=', b'AB'), (b'QU JD\n', b'ABC'), (b'QUJ', None),
                       (b'QU*D', None), (b'Q=JD', None), (b'QUI=QUJD', None)]:
        recs.append(MC.corpus_record(text, False, 16, want))
    corpus = tmp_path / 'corpus.bin'
    corpus.write_bytes(b''.join(recs))
    # (out-of-range accesses and undefined behaviour are what is looked for; the leak check at exit needs ptrace)
    run = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert f'{len(recs)} records, 0 mismatches' in run.stdout


# ---------------------------------------------------------------------------------------------- the restatement
def _one(**kw):
    mz, it = np.array([100.5, 200.25, 300.125]), np.array([1.0, 2.0, 3.0])
    return MC.spectrum(0, mz, it, **kw)


def test_restatement_reads_the_named_cases(caplog):
    rng = np.random.default_rng(1)
    mz, it = MC.peaks(rng, 5)
    spectra = [MC.spectrum(0, mz, it, level=1, rt='0.1'),
               MC.spectrum(1, mz, it, charge=3, rt='1.25', pmz='444.5', f64=(True, False), z=(True, False)),
               MC.spectrum(2, mz, it, charge=None, possible=(2,), sid='index=7'),
               MC.spectrum(3, mz, it, charge=None, precursors=2, ions=2),
               MC.spectrum(4, mz, it, level=3),
               MC.spectrum(5, mz, it, sid='no number here'),
               MC.spectrum(6, mz[::-1], it, sid='a&amp;b scan=12', q="'")]
    with caplog.at_level(logging.WARNING):
        got = mzml_ref.read_mzml(MC.document(spectra))
    assert [(s.index, s.identifier, s.precursor_charge) for s in got] == \
        [(1, '2', 3), (2, '7', 2), (3, '4', None), (6, '12', 2)]
    assert (got[0].precursor_mz, got[0].retention_time) == (444.5, 1.25)
    assert got[0].mz.dtype == np.float64 and got[0].intensity.dtype == np.float32
    assert np.array_equal(got[0].mz, mz) and np.array_equal(got[0].intensity, it.astype(np.float32))
    assert got[2].precursor_mz == 500.5 and got[2].retention_time == 1.5        # the first precursor, ion and scan
    assert np.array_equal(got[3].mz, mz[::-1])                                  # (pack_raw sorts)
    assert sum('failed to read spectrum' in r.message for r in caplog.records) == 1
    assert mzml_ref.read_mzml(MC.document(spectra, newlines=False))[1].identifier == '7'


@pytest.mark.parametrize('change, text', [
    (dict(rt=None), 'spectrum 0: no scan start time'),
    (dict(pmz=None), 'spectrum 0: no precursor'),
    (dict(precursors=0), 'spectrum 0: no precursor'),
    (dict(charge=None, possible=(2, 3)), 'spectrum 0: several possible'),
    (dict(charge='2+'), 'spectrum 0: charge'),
    (dict(dal=4), 'spectrum 0: 24 bytes'),
    (dict(dal=2), 'spectrum 0'),
    (dict(head='<referenceableParamGroupRef ref="g"/>'), 'spectrum 0: a referenceableParamGroupRef'),
    (dict(inside='<!-- late -->'), 'spectrum 0: a comment'),
    (dict(rt='soon'), "spectrum 0: scan start time 'soon'"),
])
def test_restatement_refuses(change, text):
    with pytest.raises(ValueError, match=text):
        mzml_ref.read_mzml(MC.document([_one(**change)]))


def test_restatement_refuses_arrays():
    mz, it = np.array([100.5, 200.25, 300.125]), np.array([1.0, 2.0, 3.0])
    good = MC.array(it, 'it')
    stream = bytearray(MC.deflate(mz.tobytes()))
    stream[-1] ^= 1
    for arrays in ([MC.array(mz, 'mz', attrs=' arrayLength="3"'), good],
                   [MC.array(mz, 'mz', precision=MC.cv('1000522', '64-bit integer')), good],
                   [MC.array(mz, 'mz', compression=MC.cv('1002312', 'MS-Numpress linear')), good],
                   [MC.array(mz, 'mz', content=base64.b64encode(bytes(stream)).decode()), good],
                   [MC.array(mz, 'mz', content='AAA*'), good],
                   [MC.array(mz, 'other'), good], [MC.array(mz, 'mz')]):
        with pytest.raises(ValueError, match='spectrum 0'):
            mzml_ref.read_mzml(MC.document([MC.spectrum(0, mz, it, arrays=arrays)]))


# ---------------------------------------------------------------------------------------------- the switch
def test_switch_and_flag():
    from ann_solo_amd import config
    assert config.Config().device_mzml is False and config.Config(device_mzml=1).device_mzml is True
    src = open(os.path.join(HERE, '..', 'ann_solo_amd', 'config.py')).read()
    assert "'--device_mzml'" in src


def test_identifier_rule_and_entities():
    from ann_solo_amd.mzml import scan_identifier, unescape
    assert scan_identifier('controllerType=0 controllerNumber=1 scan=0012') == '12'
    assert scan_identifier('index=5') == '5' and scan_identifier('scan= 7 ') == '7'
    assert scan_identifier('scan=3 index=4') is None and scan_identifier('spectrum 9') is None
    assert unescape('a&amp;b&#49;&#x32;&lt;') == 'a&b12<'
