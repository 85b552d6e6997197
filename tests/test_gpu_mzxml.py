"""The device mzXML reader (``ann_solo_amd.mzxml``, csrc/mzxml.hip) against the Python restatement of the dialect
(``tests/mzxml_ref.py``): ``read_mzxml_packed(bytes)`` must be ``pack_queries(mzxml_ref.read_mzxml(bytes))`` --
charges, tensors bit for bit, meta records with ``index`` -- and ``read_mzxml_raw(bytes)`` must be ``pack_raw`` of the
same objects, at the sizes where the scans change shape and the decode windows end, in every encoding, nesting and
layout the dialect allows and however the file is cut into chunks; each deviation raises ``ValueError`` naming the
scan; and ``Config.device_mzxml`` changes nothing a search returns. The files are generated (``tests/mzxml_cases.py``)
in the layouts the converters write: no converter-written mzXML exists where this suite runs. Malformed input only
ever leads to error codes and exceptions: no test provokes a fault."""
import base64
import logging

import numpy as np
import pytest

import mzxml_cases as XC
import mzxml_ref

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
        assert a.numpy().tobytes() == b.numpy().tobytes(), name


def check(data, lenient=False, **kw):
    """Both stages of the reader against the restatement; returns the reader's counts."""
    from ann_solo_amd import mzxml
    from ann_solo_amd.library_store import pack_queries, pack_raw
    objs = mzxml_ref.read_mzxml(data)
    # the parse
    stats = {}
    raw, rt, ids, index = mzxml.read_mzxml_raw(data, DEV, stats=stats, **kw)
    _same_pack(raw, pack_raw(objs, [o.precursor_charge or 0 for o in objs]))
    assert ids == [o.identifier for o in objs]
    assert index.tolist() == [o.index for o in objs]
    assert rt.tobytes() == np.array([o.retention_time for o in objs], np.float64).tobytes()
    # the whole reader
    cfg = _cfg(lenient)
    full = {}
    got_packs, got_meta = mzxml.read_mzxml_packed(data, cfg, DEV, stats=full, **kw)
    want_packs, want_meta = pack_queries(objs, cfg, DEV)
    assert list(got_packs) == list(want_packs) and got_meta == want_meta
    for z in want_packs:
        _same_pack(got_packs[z], want_packs[z])
        assert got_packs[z].identifiers == want_packs[z].identifiers
    keys = ('n_spectra', 'n_peaks', 'n_sorted', 'n_skipped_level', 'n_skipped_id', 'n_zlib', 'n_arrays', 'n_nested',
            'n_lines')
    assert {k: full[k] for k in keys} == {k: stats[k] for k in keys}
    assert stats['n_spectra'] - stats['n_skipped_id'] == len(objs) and stats['n_lines'] == XC.tags_of(data)
    assert stats['n_arrays'] == stats['n_spectra']
    if stats['n_skipped_id'] == 0:
        assert stats['n_nested'] == sum(o.nested for o in objs)
    stats['kept'] = sum(p.n for p in got_packs.values())
    return stats


# ---------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize('n_scans', [1, 2, 63, 64, 65, 257])
def test_scan_counts(n_scans):
    st = check(XC.flat_file(n_scans, seed=n_scans, z=True, f64=True))
    assert st['n_spectra'] == n_scans and st['n_sorted'] == 0 and st['chunks'] == 1 and st['n_nested'] == 0
    assert st['n_zlib'] == st['n_arrays'] == n_scans and st['kept'] >= n_scans and st['n_skipped_level'] == 0


def _with_tags(n_tags, n_groups, seed):
    """A nested file of exactly ``n_tags`` tags: padding elements go into the MS2 heads."""
    rng = np.random.default_rng(seed)
    pk = [XC.peaks(rng, 12) for _ in range(3 * n_groups)]

    def build(pads):
        out = []
        for g in range(n_groups):
            kids = [XC.scan(3 * g + 2 + k, *pk[3 * g + 1 + k], charge=2 + k, pad='      ',
                            head='        <userParam name="pad" value="1"/>\n' * pads[2 * g + k]) for k in range(2)]
            out.append(XC.scan(3 * g + 1, *pk[3 * g], level=1, children=kids))
        return XC.document(out)
    missing = n_tags - XC.tags_of(build([0] * (2 * n_groups)))
    assert missing >= 0
    data = build([missing // (2 * n_groups) + (1 if k < missing % (2 * n_groups) else 0) for k in range(2 * n_groups)])
    assert XC.tags_of(data) == n_tags
    return data


def test_tag_counts_around_the_scan_tile():
    from ann_solo_amd.mzxml import SCAN_TILE
    for n_tags in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE, 2 * SCAN_TILE + 1):
        st = check(_with_tags(n_tags, 2, seed=n_tags))
        assert st['n_lines'] == n_tags and st['n_spectra'] == 4 and st['n_nested'] == 4


def test_tag_count_beyond_two_scan_levels():
    from ann_solo_amd.mzxml import SCAN_TILE
    n_tags = SCAN_TILE * SCAN_TILE + 1                   # block partials of the block partials
    st = check(_with_tags(n_tags, 350, seed=5))
    assert st['n_lines'] == n_tags and st['n_spectra'] == 700 and st['n_skipped_level'] == 350


def test_text_lengths_around_the_byte_span():
    """The tag-start pass reads 16 bytes a thread: every length modulo 16, a '<' as the first and the last byte."""
    base = XC.nested_file(1, seed=77).rstrip(b'\n')
    base = base[base.index(b'<mzXML'):]                  # (blanks may not stand before an XML declaration)
    for pad in range(17):
        assert check(b' ' * pad + base)['n_spectra'] == 2


def _ramp(n):
    return 100.0 + 0.25 * np.arange(n), 1.0 + (np.arange(n) * 7919) % 1000


def test_peak_counts_up_to_the_64_kib_window():
    """2048 pairs of 64 bits are DEFLATE's 32 KiB window; 4096 are 64 KiB, the largest raw stream; 4097: capacity."""
    from ann_solo_amd import _lib
    from ann_solo_amd.mzxml import MAX_PEAKS, read_mzxml_packed
    counts = [0, 1, 2, 511, 512, 513, 2047, 2048, 2049, MAX_PEAKS]
    assert MAX_PEAKS == 4096
    scans = [XC.scan(i + 1, *_ramp(n), f64=True, z=i % 2 == 0) for i, n in enumerate(counts)]
    scans += [XC.scan(20, *_ramp(MAX_PEAKS), f64=True, z=True), XC.scan(21, *_ramp(2048), f64=False, z=True),
              XC.scan(22, *_ramp(MAX_PEAKS), f64=False, z=False), XC.scan(23, (), (), z=True)]
    st = check(XC.document(scans), lenient=True)
    assert st['n_peaks'] == sum(counts) + 2 * MAX_PEAKS + 2048 and st['kept'] == len(scans) - 2      # the empty ones
    over = XC.document([XC.scan(1, *_ramp(20)), XC.scan(2, *_ramp(MAX_PEAKS + 1))])
    with pytest.raises(_lib.AnnSoloMiError) as e:
        read_mzxml_packed(over, _cfg(True), DEV)
    assert e.value.code == _lib.ERR_CAPACITY
    with pytest.raises(OverflowError):
        mzxml_ref.read_mzxml(over)


def test_a_match_at_the_largest_distance_inside_a_64_kib_stream():
    """The last match of a 64 KiB stream reaches back 32 768 bytes into the first half: the out window is the
    inflater's history, whole."""
    stream, raw, mz, it = XC.far_stream()
    text = base64.b64encode(stream).decode()
    data = XC.document([XC.scan(1, *_ramp(7), z=True, f64=True),
                        XC.scan(2, mz, it, peaks_xml=XC.peaks_tag(f64=True, z=True, content=text), count=4096),
                        XC.scan(3, *_ramp(9), z=True, f64=True)])
    st = check(data, lenient=True)
    assert st['n_spectra'] == 3 and st['n_peaks'] == 4096 + 16 and st['n_zlib'] == 3
    from ann_solo_amd.mzxml import read_mzxml_raw
    got = read_mzxml_raw(data, DEV)[0]
    a, b = int(got.offsets[1]), int(got.offsets[2])
    assert got.intensity[a:b].cpu().numpy().tobytes() == it.astype(np.float32).tobytes()


# ---------------------------------------------------------------------------------------------- encodings
def test_precisions_and_compressions():
    rng = np.random.default_rng(3)
    scans = []
    for f64 in (True, False):
        for z in (True, False):
            for n in (1, 2, 3, 40, 301):                 # every base64 padding class, with and without zlib
                scans.append(XC.scan(len(scans) + 1, *XC.peaks(rng, n), f64=f64, z=z))
    scans.append(XC.scan(99, *XC.peaks(rng, 33), order='pairOrder'))                     # mzXML 2.x
    scans.append(XC.scan(100, *XC.peaks(rng, 33), byte_order=None, order=None, compression=''))
    scans.append(XC.scan(101, *XC.peaks(rng, 33), z=True, zlevel=0))                     # stored blocks
    scans.append(XC.scan(102, *XC.peaks(rng, 33), z=True, zlevel=9))
    st = check(XC.document(scans), lenient=True)
    assert st['n_spectra'] == 24 and st['n_zlib'] == 12 and st['n_arrays'] == 24


def test_blanks_inside_base64():
    mz, it = XC.peaks(np.random.default_rng(4), 100)
    for f64, z in ((False, False), (True, True)):
        text = XC.encode(mz, it, f64, z)
        broken = '\n' + '\n'.join(text[i:i + 61] for i in range(0, len(text), 61)) + ' \t\r\n'
        data = XC.document([XC.scan(1, mz, it, f64=f64, z=z, content=broken)])
        assert check(data)['n_spectra'] == 1


def test_descending_mz_is_sorted():
    rng = np.random.default_rng(6)
    mz, it = XC.peaks(rng, 50)
    swapped = mz.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    data = XC.document([XC.scan(1, mz[::-1], it), XC.scan(2, mz, it), XC.scan(3, swapped, it, f64=True, z=True)])
    assert check(data, lenient=True)['n_sorted'] == 2


# ---------------------------------------------------------------------------------------------- nesting
def test_nesting_and_the_index_over_all_scans():
    rng = np.random.default_rng(10)
    pk = lambda n=20: XC.peaks(rng, n)
    ms3 = lambda num: XC.scan(num, *pk(5), level=3, pad='        ')
    scans = [XC.scan(1, *pk(), pmz='401.5'),                                             # an MS2 at top level, before
             XC.scan(2, *pk(300), level=1, children=[                                    # MS1 with two MS2 siblings
                 XC.scan(3, *pk(), pmz='403.5', pad='      ', children=[ms3(4)]),        # ... the first holds an MS3
                 XC.scan(5, *pk(), pmz='405.5', pad='      ')]),
             XC.scan(6, *pk(), pmz='406.5'),                                             # ... and one after
             XC.scan(7, *pk(300), level=1),                                              # an MS1 without children
             XC.scan(8, *pk(), level=3),                                                 # another level at top level
             XC.scan(9, *pk(), level=2, children=[XC.scan(10, *pk(), pmz='410.5', pad='      ')]),   # MS2 in MS2
             XC.scan(11, *pk(), level=None),                                             # no msLevel: skipped
             '    <scan num="12" msLevel="1" peaksCount="0"/>\n',                        # self-closed: a head with nothing
             XC.scan(13, *pk(), pmz='413.5')]
    data = XC.document(scans)
    st = check(data)
    assert st['n_spectra'] == 7 and st['n_skipped_level'] == 6 and st['n_nested'] == 3
    from ann_solo_amd.mzxml import read_mzxml_raw
    raw, rt, ids, index = read_mzxml_raw(data, DEV)
    assert ids == ['1', '3', '5', '6', '9', '10', '13'] and index.tolist() == [0, 2, 4, 5, 8, 9, 12]
    assert raw.precursor_mz.tolist() == [401.5, 403.5, 405.5, 406.5, 500.5, 410.5, 413.5]
    for chunk in (700, 1500, 4000):                      # cut inside MS1 scans whose children are still to come
        cut = check(data, chunk_bytes=chunk)
        assert cut['chunks'] > 1 and cut['n_nested'] == 3 and cut['n_skipped_level'] == 6
    with pytest.raises(ValueError, match=r'mzXML: scan 11 \(index; num \'12\'\): no <peaks>'):
        read_mzxml_raw(data.replace(b'num="12" msLevel="1"', b'num="12" msLevel="2"'), DEV)     # must have a <peaks>
    with pytest.raises(ValueError, match='scan 11: no <peaks>'):
        mzxml_ref.read_mzxml(data.replace(b'num="12" msLevel="1"', b'num="12" msLevel="2"'))


def test_readw_and_msconvert_layouts():
    st = check(XC.nested_file(5, per_group=3, seed=12, ms3=True, z=True))
    assert st['n_spectra'] == 15 and st['n_skipped_level'] == 20 and st['n_nested'] == 15
    st = check(XC.flat_file(9, seed=13, every=3, f64=True))
    assert st['n_spectra'] == 9 and st['n_skipped_level'] == 3 and st['n_nested'] == 0
    rng = np.random.default_rng(12)
    scans = [XC.scan(i + 1, *XC.peaks(rng, 25), charge=(2, 3, None)[i % 3]) for i in range(5)]
    base = check(XC.document(scans))
    flat = XC.document(scans, newlines=False, index=False)
    assert b'\n' not in flat and check(flat)['n_peaks'] == base['n_peaks']
    assert check(XC.document([s.replace('"', "'") for s in scans]))['n_peaks'] == base['n_peaks']
    odd = [s.replace('polarity=', 'note="a > b" other=\'"\' polarity=').replace('<peaks ', '<peaks\n\t ')
            .replace('</precursorMz>', ' </precursorMz >') for s in scans]
    assert check(XC.document(odd))['n_peaks'] == base['n_peaks']
    empty = XC.document(scans + [XC.scan(6, (), (), peaks_xml=XC.peaks_tag(self_closing=True)),
                                 XC.scan(7, (), (), content=''), XC.scan(8, *XC.peaks(rng, 25))])
    assert check(empty, lenient=True)['n_spectra'] == 8


def test_other_ms_levels_cost_the_tag_pass_alone():
    rng = np.random.default_rng(10)
    profile = rng.uniform(0.0, 1e6, 65536)               # 1 MB of base64, uncompressed
    corrupt = XC.peaks_tag(content='not*base64', f64=True)
    kids = [XC.scan(2, *XC.peaks(rng, 30), pad='      '), XC.scan(3, *XC.peaks(rng, 12), pad='      ')]
    scans = [XC.scan(1, profile, profile, level=1, f64=True, count=99999, children=kids),
             XC.scan(4, (), (), level=1, peaks_xml=corrupt, count=5),                    # never decoded: unnoticed
             XC.scan(5, *XC.peaks(rng, 30))]
    data = XC.document(scans)
    st = check(data)
    assert st['n_spectra'] == 3 and st['n_skipped_level'] == 2
    assert check(data, chunk_bytes=1 << 20)['grown'] > 0                                 # an MS1 head fits no chunk


# ---------------------------------------------------------------------------------------------- metadata
def test_charges_identifiers_and_durations(caplog):
    rng = np.random.default_rng(11)
    pk = lambda: XC.peaks(rng, 20)
    values = ['PT0S', 'PT0.S', 'PT59.999S', 'PT1234.5678S', 'PT9007199254740991S',           # the device converts
              'PT12345678901234567890S', 'PT9007199254740993S', 'PT1M2S', 'PT1H', 'P1DT1S', 'PT1H2M3.5S',   # defers
              '12.5', '1e3', ' 12.5', '0.1234567890123456789012']                            # numerals, as written
    scans = [XC.scan(i + 1, *pk(), rt=v, charge=(None, 2, 3, 255)[i % 4]) for i, v in enumerate(values)]
    st = check(XC.document(scans))
    assert st['n_spectra'] == len(values)
    ids = [' 7 ', '+7', '007', '7.0', 'seven', '', '1_0', '&#x37;']
    scans = [XC.scan(v, *pk(), charge=None if i % 2 else 4) for i, v in enumerate(ids)] + \
        [XC.scan('x9', *pk(), rt=None, pmz=None)]                                            # dropped before its fields
    with caplog.at_level(logging.WARNING):
        st = check(XC.document(scans))
    assert st['n_spectra'] == 9 and st['n_skipped_id'] == 4
    assert sum('failed to read scan' in r.message for r in caplog.records) >= 8
    from ann_solo_amd.mzxml import read_mzxml_packed, read_mzxml_raw
    raw, rt, got, index = read_mzxml_raw(XC.document(scans), DEV)
    assert got == ['7', '7', '7', '10', '7'] and index.tolist() == [0, 1, 2, 6, 7]
    assert raw.precursor_charge.tolist() == [4, 0, 4, 4, 0]
    packs, meta = read_mzxml_packed(XC.document(scans), _cfg(True), DEV)
    assert sorted(packs) == [2, 3, 4] and [m['index'] for m in meta[2]] == [1, 7] == [m['index'] for m in meta[3]]


def test_precursor_numerals_at_the_edges_of_the_rule():
    """What asl_mgf_number converts, and what it defers to Python's float()."""
    values = ['500.25', '0500.250', '5.0025e2', '+500.25', '9007199254740993', '1234567890.12345678901', '4.5e-23',
              '1e23', '.5e3', '500.', ' 500.25 ', '\n  500.25\n', '5_00.25', '&#53;00.25']
    rng = np.random.default_rng(9)
    scans = [XC.scan(i + 1, *XC.peaks(rng, 12), pmz=v) for i, v in enumerate(values)]
    assert check(XC.document(scans))['n_spectra'] == len(values)


# ---------------------------------------------------------------------------------------------- every cut
_KID = ('<scan num="%d" msLevel="2" peaksCount="2" retentionTime="PT%d.5S"><precursorMz precursorCharge="2">44%d.5'
        '</precursorMz><peaks precision="32">%s</peaks></scan>')
_GROUP = '<scan num="%d" msLevel="1" peaksCount="2" retentionTime="PT%dS"><peaks precision="32">%s</peaks>%s%s</scan>'


def test_every_cut_across_one_nested_group():
    """The same result wherever the first chunk ends inside an MS1 scan that holds two MS2 scans."""
    from ann_solo_amd import mzxml
    two = lambda k: XC.encode([100.5 + k, 200.25 + k], [7.0 + k, 3.0])
    kid = lambda num: _KID % (num, num, num, two(num))
    group = lambda num: _GROUP % (num, num, two(0), kid(num + 1), kid(num + 2))
    data = ('<mzXML><msRun>' + group(1) + group(4) + '</msRun></mzXML>').encode()
    assert len(data) < 1100
    check(data)
    whole = mzxml.read_mzxml_raw(data, DEV)
    a, b = data.index(b'<scan num="4"'), data.rindex(b'</scan>') + 7
    assert 300 < b - a < 600 and whole[2] == ['2', '3', '5', '6']
    for cut in range(a - 1, b + 2):
        st = {}
        raw, rt, ids, index = mzxml.read_mzxml_raw(data, DEV, chunk_bytes=cut, stats=st)
        assert st['chunks'] >= 2 and st['n_nested'] == 4 and st['n_skipped_level'] == 2, cut
        _same_pack(raw, whole[0])
        assert ids == whole[2] and index.tolist() == [1, 2, 4, 5] and rt.tobytes() == whole[1].tobytes(), cut
    for cut in (1, 50):                                   # chunks that close nothing are doubled
        st = {}
        _same_pack(mzxml.read_mzxml_raw(data, DEV, chunk_bytes=cut, stats=st)[0], whole[0])
        assert st['grown'] > 0
    check(XC.nested_file(22, per_group=3, seed=65), chunk_bytes=20000)


# ---------------------------------------------------------------------------------------------- errors
MZ, IT = np.array([100.5, 200.25, 300.125]), np.array([1.0, 2.0, 3.0])


def _flipped(at):
    stream = bytearray(XC.deflate(XC.pairs_bytes(MZ, IT)))
    stream[at] ^= 0x10
    return base64.b64encode(bytes(stream)).decode()


DEVIATIONS = [
    ('no retentionTime', dict(rt=None)),
    ('a duration without its S', dict(rt='PT5')),
    ('a signed duration', dict(rt='-PT5S')),
    ('a retention time that is no number', dict(rt='soon')),
    ('a non-finite retention time', dict(rt='1e400')),
    ('no precursorMz', dict(pmz=None)),
    ('a precursor that is no number', dict(pmz='heavy')),
    ('an empty precursor', dict(pmz='')),
    ('a non-finite precursor', dict(pmz='1e999')),
    ('a charge with a sign', dict(charge='2+')),
    ('charge 0', dict(charge=0)),
    ('charge 256', dict(charge=256)),
    ('a lying peaksCount, too large', dict(count=4)),
    ('a lying peaksCount, too small', dict(count=2)),
    ('a lying peaksCount, compressed, too large', dict(count=4, z=True)),
    ('a lying peaksCount, compressed, too small', dict(count=2, z=True)),
    ('peaksCount that is no number', dict(count='many')),
    ('no peaksCount', dict(count=False)),
    ('an msLevel that is no number', dict(level='two')),
    ('precision 16', dict(precision='16')),
    ('no precision', dict(precision='')),
    ('little-endian', dict(byte_order='little')),
    ('another contentType', dict(order_value='int-m/z')),
    ('another pairOrder', dict(order='pairOrder', order_value='intensity')),
    ('another compression', dict(compression='gzip')),
    ('two peaks', dict(peaks_xml=XC.peaks_tag(MZ, IT) + XC.peaks_tag(MZ, IT))),
    ('no peaks', dict(peaks_xml='')),
    ('a stray byte in base64', dict(content='AAA*')),
    ('base64 of a bad length', dict(content=XC.encode(MZ, IT)[:-1])),
    ('padding inside base64', dict(content='AA==' + XC.encode(MZ, IT))),
    ('a stream that is not compressed', dict(z=True, content=XC.encode(MZ, IT))),
    ('a corrupt zlib stream', dict(z=True, content=_flipped(6))),
    ('a wrong Adler-32', dict(z=True, content=_flipped(-1))),
    ('a bad zlib header', dict(z=True, content=_flipped(0))),
    ('a truncated stream', dict(z=True, content=base64.b64encode(XC.deflate(XC.pairs_bytes(MZ, IT))[:-3]).decode())),
    ('an empty compressed stream', dict(z=True, content='')),
    ('a comment', dict(inside='<!-- late -->')),
    ('a CDATA section', dict(inside='<userParam><![CDATA[x]]></userParam>')),
    ('peaks behind a child scan', dict(inside='<peaks precision="32"></peaks>',
                                       children=[XC.scan(5, MZ, IT, level=3, pad='      ')])),
    ('a precursor behind a child scan', dict(inside='<precursorMz>5.5</precursorMz>',
                                             children=[XC.scan(5, MZ, IT, level=3, pad='      ')])),
]


@pytest.mark.parametrize('name, change', DEVIATIONS, ids=[d[0] for d in DEVIATIONS])
def test_deviations_raise_value_errors_that_name_the_scan(name, change):
    from ann_solo_amd import mzxml
    rng = np.random.default_rng(13)
    good = [XC.scan(i, *XC.peaks(rng, 12)) for i in (1, 2, 9)]
    survey = XC.scan(3, *XC.peaks(rng, 40), level=1, children=[XC.scan(4, MZ, IT, pad='      ', **change)])
    data = XC.document(good[:2] + [survey] + good[2:])
    outside = 'behind a child scan' in name              # named by the scan in front of the tag: the child
    where = 'scan 4' if outside else 'scan 3'
    with pytest.raises(ValueError, match=where):
        mzxml_ref.read_mzxml(data)
    num = '' if outside or name in ('a comment', 'a CDATA section', 'an msLevel that is no number') else r"num '4'\)"
    for chunk in (256 << 20, 3000):
        with pytest.raises(ValueError, match=rf'mzXML: {where} \(index; .*{num}'):
            mzxml.read_mzxml_packed(data, _cfg(True), DEV, chunk_bytes=chunk)
    with pytest.raises(ValueError, match=rf'mzXML: {where} \(index; .*{num}'):
        mzxml.read_mzxml_raw(data, DEV)


def test_decode_failures_carry_the_inflaters_text():
    from ann_solo_amd import _lib, mzxml
    for change, code in ((dict(z=True, content=_flipped(-1)), 13), (dict(content='AAA*'), 1),
                         (dict(count=4), 14), (dict(count=2), 12), (dict(z=True, content=_flipped(0)), 5)):
        with pytest.raises(ValueError) as e:
            mzxml.read_mzxml_raw(XC.document([XC.scan(1, MZ, IT, **change)]), DEV)
        assert str(e.value) == f"mzXML: scan 0 (index; num '1'): peaks: {_lib.MZML_INF_TEXT[code]}"
    data = XC.document([XC.scan(1, MZ, IT)]).replace(b'num="1"', b'')
    with pytest.raises(ValueError, match=r'mzXML: scan 0 \(index; num None\): no num attribute'):
        mzxml.read_mzxml_raw(data, DEV)
    with pytest.raises(ValueError, match='scan 0: no num'):
        mzxml_ref.read_mzxml(data)


def test_a_tag_beyond_the_cap_is_an_error_code_not_a_long_walk():
    from ann_solo_amd import _lib, mzxml
    ok = XC.scan(1, MZ, IT, head='<userParam name="%s"/>' % ('x' * (mzxml.MAX_TAG - 20)))
    assert check(XC.document([ok]))['n_spectra'] == 1
    long = XC.scan(1, MZ, IT, head='<userParam name="%s"/>' % ('x' * mzxml.MAX_TAG))
    with pytest.raises(_lib.AnnSoloMiError) as e:
        mzxml.read_mzxml_packed(XC.document([long]), _cfg(), DEV)
    assert e.value.code == _lib.ERR_CAPACITY


def test_an_unclosed_last_head_and_empty_inputs(caplog):
    from ann_solo_amd import mzxml
    data = XC.flat_file(3, seed=14)
    cut = data[:data.rindex(b'</scan>')]
    with caplog.at_level(logging.WARNING):
        raw, rt, ids, index = mzxml.read_mzxml_raw(cut, DEV)
    assert ids == ['1', '2'] and any('not closed' in r.message for r in caplog.records)
    nested = XC.nested_file(1, seed=14)
    cut = nested[:nested.index(b'</scan>')]              # the first MS2 head is open; the MS1 head before it is closed
    assert mzxml.read_mzxml_raw(cut, DEV)[2] == []
    cut = nested[:nested.index(b'</scan>') + 7]
    assert mzxml.read_mzxml_raw(cut, DEV)[2] == ['2']
    for empty in (b'', b'no tag at all', b'<mzXML></mzXML>', XC.document([])):
        raw, rt, ids, index = mzxml.read_mzxml_raw(empty, DEV)
        assert raw.n == 0 and ids == [] and len(rt) == 0
        assert mzxml.read_mzxml_packed(empty, _cfg(), DEV) == ({}, {})


# ---------------------------------------------------------------------------------------------- the search
def _mzxml_of(q):
    """The packed queries ``q`` as a nested mzXML file: float64 zlib streams, the charge stated, three MS2 scans to
    an MS1 scan."""
    o, mz, it = q.offsets.numpy(), q.mz.numpy().astype(np.float64), q.intensity.numpy().astype(np.float64)
    pmz, pz = q.precursor_mz.numpy(), q.precursor_charge.numpy()
    kid = lambda i, num: XC.scan(num, mz[o[i]:o[i + 1]], it[o[i]:o[i + 1]], pmz=repr(float(pmz[i])), f64=True, z=True,
                                 charge=int(pz[i]), rt='PT%.3fS' % (0.6 * i), pad='      ')
    out, num = [], 1
    for a in range(0, q.n, 3):
        kids = [kid(i, num + 1 + i - a) for i in range(a, min(a + 3, q.n))]
        out.append(XC.scan(num, MZ, IT, level=1, children=kids))
        num += 1 + len(kids)
    return XC.document(out)


def test_search_with_the_switch_is_search_without_it(tmp_path):
    from ann_solo_amd import synthetic
    from ann_solo_amd.library_store import pack_queries
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, aux = synthetic.make_library(3000, seed=41, device='cpu', charges=(2, 3), charge_p=(0.7, 0.3))
    q, _ = synthetic.make_queries(lib, aux, 200, seed=42, open_range=300.0)
    path = tmp_path / 'Queries.mzXML'                    # the extension in any letter case
    path.write_bytes(_mzxml_of(q))
    kw = dict(num_list=16, num_probe=8, num_candidates=256, index='ivfpq', kmeans_niter=4, batch_size=64)
    tables, called = [], []
    for device_mzxml in (True, False):
        def reader(filename):
            assert not device_mzxml, 'the switch is on: the query reader must not be called'
            called.append(filename)
            return mzxml_ref.read_mzxml(filename)
        sl = SpectralLibrary(lib, config=Config.open_search(device_mzxml=device_mzxml, **kw), device=DEV,
                             query_reader=reader)
        lmeta = {z: [dict(identifier=int(r), peptide=f'P{r}K', precursor_mz=float(p), is_decoy=False)
                     for r, p in enumerate(part.precursor_mz)] for z, part in sl.partitions.items()}
        t = sl.search(str(path), library_meta=lmeta)
        tables.append((t, [(s.query_identifier, s.query_index, s.retention_time) for s in t]))
        if not device_mzxml:     # and the switch off is the path as it was: the packed driver over pack_queries
            qs, qm = pack_queries(mzxml_ref.read_mzxml(str(path)), sl.config, DEV)
            tables.append((sl.search(qs, qm, lmeta), None))
        sl.shutdown()
    assert called == [str(path)]                         # off: the .mzXML name went to query_reader as before
    (on, on_ids), (off, off_ids), (packed, _) = tables
    assert len(on) > 100 and on_ids == off_ids
    for t in (off, packed):
        for col in ('charge', 'qrow', 'lib_row', 'score', 'q'):
            a, b = np.asarray(getattr(on, col)), np.asarray(getattr(t, col))
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), col
