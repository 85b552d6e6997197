"""The device MGF reader (``ann_solo_amd.mgf``, csrc/mgf.hip) against the Python restatement of the dialect
(``tests/mgf_ref.py``): ``read_mgf_packed(bytes)`` must be ``pack_queries(mgf_ref.read_mgf(bytes))`` -- charges,
tensors bit for bit, meta records -- and ``read_mgf_raw(bytes)`` must be ``pack_raw`` of the same objects, at the
sizes where the scans change shape, in every form the dialect allows, in any order of the peaks, at the edges of
the numeral rule and however the file is cut into chunks; each deviation raises ``ValueError`` naming the line
or spectrum; and ``Config.device_mgf`` changes nothing a search returns. Malformed text only ever leads to error
codes and exceptions: no test provokes a fault."""
import logging

import numpy as np
import pytest
import torch

import mgf_cases as MC
import mgf_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _cfg(lenient=False):
    from ann_solo_amd.config import Config
    if lenient:      # every spectrum with a peak in range survives, up to 256 peaks of it
        return Config(min_peaks=1, min_mz_range=0.0, min_intensity=0.0, max_peaks_used=256, min_mz=1, max_mz=5000)
    return Config()


def _same_pack(g, w):
    for name in ('offsets', 'mz', 'intensity', 'charge', 'precursor_mz', 'precursor_charge'):
        a, b = getattr(g, name).cpu(), getattr(w, name).cpu()
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(a, b) and a.numpy().tobytes() == b.numpy().tobytes(), name


def check(data, lenient=False, **kw):
    """Both stages of the reader against the restatement; returns the reader's counts."""
    from ann_solo_amd import mgf
    from ann_solo_amd.library_store import pack_queries, pack_raw
    objs = mgf_ref.read_mgf(data)
    # the parse
    stats = {}
    raw, rt, ids = mgf.read_mgf_raw(data, DEV, stats=stats, **kw)
    want = pack_raw(objs, [o.precursor_charge or 0 for o in objs])
    _same_pack(raw, want)
    assert ids == [o.identifier for o in objs]
    want_rt = np.array([np.nan if o.retention_time is None else o.retention_time for o in objs], np.float64)
    assert rt.tobytes() == want_rt.tobytes()
    # the whole reader
    cfg = _cfg(lenient)
    full = {}
    got_packs, got_meta = mgf.read_mgf_packed(data, cfg, DEV, stats=full, **kw)
    want_packs, want_meta = pack_queries(objs, cfg, DEV)
    assert list(got_packs) == list(want_packs) and list(got_meta) == list(want_meta)
    assert got_meta == want_meta
    for z in want_packs:
        _same_pack(got_packs[z], want_packs[z])
        assert got_packs[z].identifiers == want_packs[z].identifiers
    assert {k: full[k] for k in ('n_spectra', 'n_peaks', 'n_deferred', 'n_sorted')} == \
        {k: stats[k] for k in ('n_spectra', 'n_peaks', 'n_deferred', 'n_sorted')}
    assert stats['n_spectra'] == len(objs)
    stats['kept'] = sum(p.n for p in got_packs.values())
    return stats


# ---------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize('n_spectra', [1, 2, 63, 64, 65, 257])
def test_spectrum_counts(n_spectra):
    st = check(MC.plain_file(n_spectra, seed=n_spectra))
    assert st['n_deferred'] == 0 and st['n_sorted'] == 0 and st['chunks'] == 1
    assert st['kept'] >= n_spectra                       # (every spectrum survives; unknown charges twice)


def test_line_counts_around_the_scan_tile():
    from ann_solo_amd.mgf import SCAN_TILE
    for n_lines in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE, 2 * SCAN_TILE + 1):
        st = check(MC.file_of_lines(n_lines, seed=n_lines))
        assert st['n_lines'] == n_lines and st['n_deferred'] == 0 and st['n_sorted'] == 0


def test_line_count_beyond_two_scan_levels():
    from ann_solo_amd.mgf import SCAN_TILE
    n_lines = SCAN_TILE * SCAN_TILE + 1                  # block partials of the block partials
    st = check(MC.file_of_lines(n_lines, seed=5))
    assert st['n_lines'] == n_lines and st['n_deferred'] == 0


def test_text_lengths_around_the_byte_span():
    """The line-start pass reads 16 bytes a thread: every length modulo 16, with and without a final newline."""
    base = MC.plain_file(3, seed=77).rstrip(b'\n')
    for pad in range(17):
        check(b' ' * pad + base)
        check(b' ' * pad + base + b'\n')


def _block(title, peaks, extra=()):
    lines = ['BEGIN IONS', f'TITLE={title}', 'PEPMASS=500.5', 'CHARGE=2+', *extra]
    return '\n'.join(lines + ['%s %s' % p for p in peaks] + ['END IONS']) + '\n'


def _ramp(n, lo=100.0, step=0.25):
    return [('%.2f' % (lo + step * i), '%d' % (1 + (i * 7919) % 1000)) for i in range(n)]


def test_empty_and_full_spectra():
    from ann_solo_amd import _lib
    from ann_solo_amd.mgf import MAX_PEAKS, read_mgf_packed
    data = (_block('none', []) + _block('full', _ramp(MAX_PEAKS)) + _block('some', _ramp(20))).encode()
    st = check(data, lenient=True)
    assert st['n_peaks'] == MAX_PEAKS + 20 and st['n_sorted'] == 0 and st['kept'] == 2      # 'none' is dropped
    over = (_block('some', _ramp(20)) + _block('over', _ramp(MAX_PEAKS + 1))).encode()
    with pytest.raises(_lib.AnnSoloMiError) as e:
        read_mgf_packed(over, _cfg(True), DEV)
    assert e.value.code == _lib.ERR_CAPACITY


# ---------------------------------------------------------------------------------------------- form
def test_crlf_and_no_final_newline():
    data = MC.plain_file(5, seed=3, newline='\r\n')
    assert check(data)['n_deferred'] == 0
    assert check(data.rstrip(b'\r\n'))['n_spectra'] == 5
    assert check(MC.plain_file(5, seed=3).rstrip(b'\n'))['n_spectra'] == 5


def test_blank_lines_comments_order_duplicates_and_odd_values(caplog):
    body = ['%.4f %.2f' % (100.0 + 35.0625 * i, 1.0 + (i * 37) % 97) for i in range(40)]   # 12 of them span 385 m/z
    text = '\n'.join([
        '# produced by hand', 'CHARGE=2+ and 3+', 'COM=a header line', '', 'text before the first block', 'END IONS',
        'BEGIN IONS', '', '# a comment', 'RTINSECONDS=10.5', *body[:10], 'CHARGE=3+', 'PEPMASS=400.25 1e5 3+',
        '; another', 'TITLE=a title = with = signs', *body[10:20], 'USER00=', '/ slash', '! bang', 'END IONS',
        'text between', 'KEY=outside a block', 'END IONS', '',
        '  BEGIN IONS  ', 'pepmass=1.5', 'Title=mentions END IONS inside', 'PEPMASS=600.125', *body[:15],
        '\t END IONS \t',
        'BEGIN IONS', 'SCAN=41', 'TITLE=', 'PEPMASS=700', 'charge=2,3', 'CHARGE=', 'Charge=2,3', *body[5:25], 'END IONS',
        'BEGIN IONS', 'SCAN=42', 'PEPMASS=\t800.5\t', 'RTINSECONDS= 7 ', *['  %s  extra tokens 2+' % b for b in body[:12]],
        'END IONS', 'text after', 'BEGIN IONS', 'TITLE=never closed', 'PEPMASS=1', *body[:12]]).encode()
    with caplog.at_level(logging.WARNING):
        st = check(text)
    assert sum('not closed' in r.message for r in caplog.records) >= 2      # the restatement and the reader
    assert st['n_spectra'] == 4 and st['n_deferred'] == 0 and st['kept'] == 4    # (the header's charge: none unknown)
    from ann_solo_amd.mgf import read_mgf_packed
    packs, meta = read_mgf_packed(text, _cfg(), DEV)
    assert list(packs) == [3, 2]
    assert [m['identifier'] for m in meta[3]] == ['a title = with = signs']
    assert [(m['identifier'], m['precursor_mz'], m['retention_time']) for m in meta[2]] == \
        [('mentions END IONS inside', 600.125, None), ('', 700.0, None), ('42', 800.5, 7.0)]


def test_header_defaults_of_every_parameter():
    rng = np.random.default_rng(12)
    blocks = ''.join(MC.spectrum_block(rng, f's{i}', charge=None, rt=False) for i in range(3))
    body = blocks.replace('TITLE=s1\n', 'SCAN=5\n').replace('TITLE=s2\n', '')
    second = body.index('PEPMASS', body.index('SCAN=5'))
    body = body[:second] + body[body.index('\n', second) + 1:]          # block 2 takes the header's pepmass
    text = ('TITLE=from the header\nPEPMASS=444.5 2\nCHARGE=3+\nRTINSECONDS=99.5\n' + body).encode()
    st = check(text)
    assert st['n_spectra'] == 3
    from ann_solo_amd.mgf import read_mgf_packed
    _, meta = read_mgf_packed(text, _cfg(), DEV)
    # the header's title goes before a block's scan, as in a dict the block updates
    assert [m['identifier'] for m in meta[3]] == ['s0', 'from the header', 'from the header']
    assert meta[3][1]['precursor_mz'] == 444.5 and meta[3][0]['precursor_mz'] != 444.5
    assert [m['retention_time'] for m in meta[3]] == [99.5] * 3


def test_charges():
    rng = np.random.default_rng(13)
    charges = ['3+', '2,3', None, '2', '+4', '5+ and 6+', '2+and3+', ' 7 ']
    text = ''.join(MC.spectrum_block(rng, f'c{i}', charge=c) for i, c in enumerate(charges)).encode()
    st = check(text)
    assert st['kept'] == len(charges) + 1
    from ann_solo_amd.mgf import read_mgf_packed
    packs, _ = read_mgf_packed(text, _cfg(), DEV)
    assert list(packs) == [3, 2, 4, 5, 7]                # first appearance; the unknown one at 2 and 3


# ---------------------------------------------------------------------------------------------- order
def test_one_descending_pair_and_a_fully_reversed_spectrum():
    from ann_solo_amd.mgf import MAX_PEAKS
    up = _ramp(30)
    swapped = list(up)
    swapped[11], swapped[12] = swapped[12], swapped[11]
    data = (_block('up', up) + _block('pair', swapped) + _block('up2', _ramp(64)) +
            _block('reversed', _ramp(MAX_PEAKS)[::-1]) + _block('rev2', _ramp(2)[::-1]) +
            _block('rev65', _ramp(65)[::-1])).encode()
    st = check(data, lenient=True)
    assert st['n_sorted'] == 4 and st['n_deferred'] == 0


def test_ties_after_float32_rounding_keep_file_order():
    # 500.000002 and 500.000001 descend as doubles and tie as float32: no sort for them alone ...
    # (and -0.0 does not descend from 0.0)
    zeros = [('0.0', '4'), ('-0.0', '5'), ('-0', '6')]
    ties = [('500.000002', '1'), ('500.000001', '2'), ('500.000003', '3')]
    st = check(_block('ties', zeros + [('400.5', '9')] + ties + [('600.5', '8')]).encode(), lenient=True)
    assert st['n_sorted'] == 0
    # ... and inside a spectrum that is sorted they keep their order
    st = check((_block('ties', [('700.5', '9')] + ties + zeros + [('600.5', '8'), ('0', '7')]) +
                _block('up', _ramp(12))).encode(), lenient=True)
    assert st['n_sorted'] == 1


# ---------------------------------------------------------------------------------------------- numerals
def _numeral_file(tokens):
    blocks = []
    for i in range(0, len(tokens), 6):
        part = tokens[i:i + 6]
        peaks = [(t.decode(), '1.5') for t in part] + [('2.5', t.decode()) for t in part]
        blocks.append(_block(f'n{i}', peaks, extra=['PEPMASS=' + part[0].decode() + ' 1e999 x',
                                                    'RTINSECONDS=' + part[-1].decode()]))
    return ''.join(blocks).encode('latin-1')


def test_edge_numerals_in_peaks_pepmass_and_retention_time():
    tokens = [t for t in MC.EDGES if t not in MC.REFUSED and t not in MC.NON_FINITE and t != b'1.7976931348623157e308']
    data = _numeral_file(tokens)
    want = 0
    for i in range(0, len(tokens), 6):
        part = tokens[i:i + 6]
        want += 2 * sum(map(MC.needs_host, part)) + MC.needs_host(part[0]) + MC.needs_host(part[-1])
        want += MC.needs_host(b'500.5')                  # (the block's own PEPMASS line, overridden: converted)
    assert 10 < want < 4 * len(tokens)
    st = check(data, lenient=True)
    assert st['n_deferred'] == want and st['n_spectra'] == (len(tokens) + 5) // 6
    ordinary = [t for t in tokens if not MC.needs_host(t)]
    assert check(_numeral_file(ordinary), lenient=True)['n_deferred'] == 0


def test_random_numerals_in_a_file():
    tokens = MC.random_numerals(3000, seed=21)
    st = check(_numeral_file(tokens), lenient=True)
    assert 0 < st['n_deferred'] < 0.5 * 14 * len(tokens) / 6


# ---------------------------------------------------------------------------------------------- chunking
def test_chunk_cuts_and_growth():
    from ann_solo_amd import mgf
    data = MC.plain_file(65, seed=65)
    cfg = _cfg()
    base = {}
    one = mgf.read_mgf_packed(data, cfg, DEV, stats=base)
    assert base['chunks'] == 1 and base['grown'] == 0
    behind_end = data.index(b'END IONS\n', len(data) // 3) + len(b'END IONS\n')
    in_numeral = data.index(b'.', behind_end + 80) + 2
    assert data[in_numeral - 1:in_numeral + 1].isdigit()
    in_block = data.index(b'\n', in_numeral) + 1
    assert not data[in_block:].startswith(b'BEGIN') and not data[in_block:].startswith(b'END')
    for cut, grows in ((in_numeral, False), (in_block, False), (behind_end, False), (4096, False), (64, True), (1, True)):
        st = {}
        packs, meta = mgf.read_mgf_packed(data, cfg, DEV, chunk_bytes=cut, stats=st)
        assert (st['grown'] > 0) == grows and st['chunks'] > 1
        assert st['n_spectra'] == 65 and st['n_lines'] == base['n_lines'] and st['n_peaks'] == base['n_peaks']
        assert meta == one[1] and list(packs) == list(one[0])
        for z in packs:
            _same_pack(packs[z], one[0][z])
    check(data, chunk_bytes=in_numeral)
    check(b'CHARGE=3+\n\n' + data.replace(b'CHARGE=2+\n', b''), chunk_bytes=5000)     # the header is kept across chunks


# ---------------------------------------------------------------------------------------------- errors
_GOOD = _block('good', _ramp(12))
_DEVIATIONS = [
    ('one token', _block('bad', _ramp(3) + [('150.5', '')]), 'line', 8),
    ('nested', 'BEGIN IONS\nTITLE=x\nPEPMASS=1\n1 2\nBEGIN IONS\n1 2\nEND IONS\n', 'line', 5),
    ('float refuses m/z', _block('bad', [('1', '2'), ('1,5', '2')]), 'line', 6),
    ('float refuses intensity', _block('bad', [('1', '2'), ('3', '4x')]), 'line', 6),
    ('non-finite m/z', _block('bad', [('nan', '2')]), 'line', 5),
    ('non-finite intensity', _block('bad', [('1', '1e999')]), 'line', 5),
    ('no pepmass', 'BEGIN IONS\nTITLE=x\n1 2\nEND IONS\n', 'spectrum', 3),
    ('no title, no scan', 'BEGIN IONS\nPEPMASS=5\n1 2\nEND IONS\n', 'spectrum', 3),
    ('non-finite pepmass', 'BEGIN IONS\nTITLE=x\nPEPMASS=inf\n1 2\nEND IONS\n', 'spectrum', 3),
    ('empty pepmass', 'BEGIN IONS\nTITLE=x\nPEPMASS=\n1 2\nEND IONS\n', 'spectrum', 3),
    ('pepmass float refuses', 'BEGIN IONS\nTITLE=x\nPEPMASS=12,5 3\n1 2\nEND IONS\n', 'spectrum', 3),
    ('charge 0', 'BEGIN IONS\nTITLE=x\nPEPMASS=5\nCHARGE=0\n1 2\nEND IONS\n', 'spectrum', 3),
    ('charge 256', 'BEGIN IONS\nTITLE=x\nPEPMASS=5\nCHARGE=256\n1 2\nEND IONS\n', 'spectrum', 3),
    ('charge 2-', 'BEGIN IONS\nTITLE=x\nPEPMASS=5\nCHARGE=2-\n1 2\nEND IONS\n', 'spectrum', 3),
    ('charge word', 'BEGIN IONS\nTITLE=x\nPEPMASS=5\nCHARGE=two\n1 2\nEND IONS\n', 'spectrum', 3),
    ('retention time', 'BEGIN IONS\nTITLE=x\nPEPMASS=5\nRTINSECONDS=1 2\n1 2\nEND IONS\n', 'spectrum', 3),
]


@pytest.mark.parametrize('name, bad, unit, number', _DEVIATIONS, ids=[d[0] for d in _DEVIATIONS])
def test_deviations_raise_value_errors_that_name_the_place(name, bad, unit, number):
    from ann_solo_amd import mgf
    head = 'junk\n' + _GOOD + '\n' + _GOOD                # 2 spectra, 2 * 17 + 2 = 36 lines
    assert head.count('\n') == 36
    where = number + 36 if unit == 'line' else number
    data = (head + bad + _GOOD).encode()
    with pytest.raises(ValueError, match=f'{unit} {where}:'):
        mgf_ref.read_mgf(data)
    for chunk in (1 << 20, 300):                         # the numbers are the file's, not the chunk's
        with pytest.raises(ValueError, match=f'{unit} {where}:'):
            mgf.read_mgf_packed(data, _cfg(True), DEV, chunk_bytes=chunk)
        with pytest.raises(ValueError, match=f'{unit} {where}:'):
            mgf.read_mgf_raw(data, DEV, chunk_bytes=chunk)
    check((head + _GOOD).encode(), lenient=True)         # the reader works on after a failed call


def test_the_first_deviation_in_file_order_is_reported():
    from ann_solo_amd import mgf
    no_pepmass = 'BEGIN IONS\nTITLE=x\n1 2\nEND IONS\n'
    one_token = _block('bad', [('150.5', '')])
    for data, want in (((no_pepmass + one_token).encode(), 'spectrum 1:'), ((one_token + no_pepmass).encode(), 'line 5:')):
        with pytest.raises(ValueError, match=want):
            mgf_ref.read_mgf(data)
        with pytest.raises(ValueError, match=want):
            mgf.read_mgf_packed(data, _cfg(True), DEV)


_OPEN_BLOCK = 'BEGIN IONS\nTITLE=open\nPEPMASS=7\n%s\n3 4'


@pytest.mark.parametrize('line, where', [('1 2x', 'line 40:'), ('1e999 2', 'line 40:'), ('5', 'line 40:'),
                                         ('BEGIN IONS', 'line 40:'), ('1 2\n1e23 0x', 'line 41:')])
def test_deviations_in_an_unclosed_last_block_are_reported_like_any_other(line, where):
    """The restatement reads line by line: it meets a bad line of the last block before it meets the end of the
    file. Numerals the device defers are no exception."""
    from ann_solo_amd import mgf
    data = ('\n\n' + _GOOD + _GOOD + _OPEN_BLOCK % line).encode()       # 2 + 2 * 17 + 3 = 39 lines before it
    with pytest.raises(ValueError, match=where):
        mgf_ref.read_mgf(data)
    for chunk in (1 << 20, 300):
        with pytest.raises(ValueError, match=where):
            mgf.read_mgf_packed(data, _cfg(True), DEV, chunk_bytes=chunk)
    only = (_OPEN_BLOCK % line).encode()                  # no closed block at all
    with pytest.raises(ValueError, match='line ' + str(int(where[5:7]) - 36) + ':'):
        mgf.read_mgf_raw(only, DEV)


def test_an_unclosed_last_block_with_sound_lines_is_dropped(caplog):
    data = (_GOOD + _OPEN_BLOCK % '1e23 12345678901234567890\nPEPMASS=1e400').encode()
    with caplog.at_level(logging.WARNING):
        st = check(data, lenient=True)
    assert st['n_spectra'] == 1 and st['n_peaks'] == 12 and any('not closed' in r.message for r in caplog.records)
    for cut in range(len(_GOOD), len(data) + 1, 7):
        check(data, lenient=True, chunk_bytes=cut)


def test_a_cut_behind_the_words_end_ions_closes_nothing():
    """A chunk's last line may be cut anywhere; what stands before the cut may read END IONS or BEGIN IONS."""
    from ann_solo_amd import mgf
    tail = _ramp(12, lo=900.0)
    for word, sound in (('END IONS=x', True), ('END IONS x', False), ('BEGIN IONS=y', True), ('BEGIN IONSz 5', False)):
        body = _block('cut', _ramp(12)).replace('END IONS\n', '')
        data = (_GOOD + body + word + '\n' + ''.join('%s %s\n' % p for p in tail) + 'END IONS\n' + _GOOD).encode()
        cut = data.index(word.encode()) + len(word.split('=')[0].split(' x')[0].split('z')[0])
        assert data[:cut].endswith(b' IONS')
        if sound:
            one = check(data, lenient=True)
            assert one['n_spectra'] == 3 and one['n_peaks'] == 12 + 24 + 12
            assert check(data, lenient=True, chunk_bytes=cut)['n_peaks'] == one['n_peaks']
        else:
            with pytest.raises(ValueError) as ref:
                mgf_ref.read_mgf(data)
            where = str(ref.value).split(':')[0]
            for chunk in (1 << 20, cut):
                with pytest.raises(ValueError, match=where + ':'):
                    mgf.read_mgf_packed(data, _cfg(True), DEV, chunk_bytes=chunk)


def test_a_line_beyond_the_cap_is_an_error_code_not_a_long_walk():
    from ann_solo_amd import _lib, mgf
    cap = _lib.MGF_MAX_LINE
    fits = _block('t' * (cap - len('TITLE=\n')), _ramp(12))
    assert max(map(len, fits.split('\n'))) + 1 == cap
    assert check((_GOOD + fits).encode(), lenient=True)['n_spectra'] == 2
    for data in ((_GOOD + fits.replace('TITLE=', 'TITLE=u')).encode(),       # one byte more
                 _GOOD.encode() + b' ' * (cap + 1) + b'\n',                   # blanks, outside a block
                 bytes(range(11, 256)) * 2000):                               # no text at all: 490 000 bytes, no newline
        for chunk in (1 << 20, 1000):
            with pytest.raises(_lib.AnnSoloMiError) as e:
                mgf.read_mgf_packed(data, _cfg(True), DEV, chunk_bytes=chunk)
            assert e.value.code == _lib.ERR_CAPACITY


def test_abi_checks_and_empty_inputs():
    from ann_solo_amd import _lib, mgf
    for data in (b'', b'\n', b'no block at all', b'BEGIN IONS\nTITLE=open\n', b'END IONS\n' * 3):
        packs, meta = mgf.read_mgf_packed(data, _cfg(), DEV)
        assert packs == {} and meta == {}
        raw, rt, ids = mgf.read_mgf_raw(data, DEV)
        assert raw.n == 0 and len(rt) == 0 and ids == []
    L = _lib.lib()
    counts = np.zeros(16, np.int64)
    host = np.frombuffer(b'BEGIN IONS\n', np.uint8)
    assert L.asl_mgf_measure(_lib.ptr(host), len(host), 1, counts.ctypes.data_as(_lib.c_i64p)) == _lib.ERR_INVALID
    text = torch.frombuffer(bytearray(b'BEGIN IONS\nTITLE=a\nPEPMASS=1\n1 2\nEND IONS\n'), dtype=torch.uint8).to(DEV)
    _lib.check(L.asl_mgf_measure(_lib.ptr(text), text.numel(), 1, counts.ctypes.data_as(_lib.c_i64p)))
    assert counts[:6].tolist() == [5, 1, 1, 0, text.numel(), 5] and counts[6] == 0 and counts[7] == -1
    other = text.clone()
    off = np.zeros(2, np.int32)
    rc = L.asl_mgf_fill(_lib.ptr(other), other.numel(), _lib.ptr(off), *([None] * 9))
    assert rc == -3                                       # ASL_ERR_STATE: not the measured chunk
    up = torch.tensor([1.0, 2.0, 3.0], device=DEV)
    n_sorted = np.zeros(1, np.int64)
    o = torch.tensor([0, 3], dtype=torch.int32, device=DEV)
    _lib.check(L.asl_mgf_sort(_lib.ptr(o), _lib.ptr(up), _lib.ptr(up.clone()), 1, 3, n_sorted.ctypes.data_as(_lib.c_i64p)))
    assert n_sorted[0] == 0


# ---------------------------------------------------------------------------------------------- end to end
def _mgf_of(q):
    o, mz, it, _, pmz, pz = q.to('cpu').numpy()
    out = []
    for i in range(q.n):
        sl = slice(o[i], o[i + 1])
        out += ['BEGIN IONS', f'TITLE=scan={i}', 'PEPMASS=%.6f' % pmz[i], 'RTINSECONDS=%.1f' % (0.5 * i)]
        if i % 10:
            out.append(f'CHARGE={int(pz[i])}+')          # every tenth: unknown, tried at 2 and 3
        out += ['%.5f %.3f' % (m, v) for m, v in zip(mz[sl], np.exp(6.0 * it[sl]))]
        out.append('END IONS')
    return ('\n'.join(out) + '\n').encode()


def test_search_with_the_switch_is_search_without_it(tmp_path):
    from ann_solo_amd import synthetic
    from ann_solo_amd.library_store import pack_queries
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, aux = synthetic.make_library(3000, seed=41, device='cpu', charges=(2, 3), charge_p=(0.7, 0.3))
    q, _ = synthetic.make_queries(lib, aux, 200, seed=42, open_range=300.0)
    path = tmp_path / 'Queries.MGF'                      # the extension in any letter case
    path.write_bytes(_mgf_of(q))
    kw = dict(num_list=16, num_probe=8, num_candidates=256, index='ivfpq', kmeans_niter=4, batch_size=64)
    tables = []
    for device_mgf in (True, False):
        def no_reader(filename):
            raise AssertionError('the switch is on: the query reader must not be called')
        sl = SpectralLibrary(lib, config=Config.open_search(device_mgf=device_mgf, **kw), device=DEV,
                             query_reader=no_reader if device_mgf else mgf_ref.read_mgf)
        lmeta = {z: [dict(identifier=int(r), peptide=f'P{r}K', precursor_mz=float(p), is_decoy=False)
                     for r, p in enumerate(part.precursor_mz)] for z, part in sl.partitions.items()}
        t = sl.search(str(path), library_meta=lmeta)
        tables.append((t, [(s.query_identifier, s.query_index, s.retention_time) for s in t]))
        if not device_mgf:       # and the switch off is the path as it was: the packed driver over pack_queries
            qs, qm = pack_queries(mgf_ref.read_mgf(str(path)), sl.config, DEV)
            tables.append((sl.search(qs, qm, lmeta), None))
        sl.shutdown()
    (on, on_ids), (off, off_ids), (packed, _) = tables
    assert len(on) > 100 and on_ids == off_ids
    for t in (off, packed):
        for col in ('charge', 'qrow', 'lib_row', 'score', 'q'):
            a, b = np.asarray(getattr(on, col)), np.asarray(getattr(t, col))
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), col
    # a name that does not end in .mgf keeps the injected reader, switch or not
    other = tmp_path / 'queries.txt'
    other.write_bytes(path.read_bytes())
    sl = SpectralLibrary(lib, config=Config.open_search(device_mgf=True, **kw), device=DEV,
                         query_reader=mgf_ref.read_mgf)
    t = sl.search(str(other), library_meta=lmeta)
    assert np.asarray(t.score).tobytes() == np.asarray(on.score).tobytes()
    sl.shutdown()
