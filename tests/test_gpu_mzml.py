"""The device mzML reader (``ann_solo_amd.mzml``, csrc/mzml.hip, csrc/inflate.hpp) against the Python restatement of
the dialect (``tests/mzml_ref.py``): ``read_mzml_packed(bytes)`` must be ``pack_queries(mzml_ref.read_mzml(bytes))``
-- charges, tensors bit for bit, meta records with ``index`` -- and ``read_mzml_raw(bytes)`` must be ``pack_raw`` of
the same objects, at the sizes where the scans and the decode kernel change shape, in every encoding and layout the
dialect allows and however the file is cut into chunks; each deviation raises ``ValueError`` naming the spectrum; and
``Config.device_mzml`` changes nothing a search returns. The files are generated (``tests/mzml_cases.py``) in the
layout the converters write: no converter-written mzML exists where this suite runs. Malformed input only ever leads
to error codes and exceptions: no test provokes a fault."""
import base64
import logging

import numpy as np
import pytest

import mzml_cases as MC
import mzml_ref

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
    from ann_solo_amd import mzml
    from ann_solo_amd.library_store import pack_queries, pack_raw
    objs = mzml_ref.read_mzml(data)
    # the parse
    stats = {}
    raw, rt, ids, index = mzml.read_mzml_raw(data, DEV, stats=stats, **kw)
    _same_pack(raw, pack_raw(objs, [o.precursor_charge or 0 for o in objs]))
    assert ids == [o.identifier for o in objs]
    assert index.tolist() == [o.index for o in objs]
    assert rt.tobytes() == np.array([o.retention_time for o in objs], np.float64).tobytes()
    # the whole reader
    cfg = _cfg(lenient)
    full = {}
    got_packs, got_meta = mzml.read_mzml_packed(data, cfg, DEV, stats=full, **kw)
    want_packs, want_meta = pack_queries(objs, cfg, DEV)
    assert list(got_packs) == list(want_packs) and got_meta == want_meta
    for z in want_packs:
        _same_pack(got_packs[z], want_packs[z])
        assert got_packs[z].identifiers == want_packs[z].identifiers
    keys = ('n_spectra', 'n_peaks', 'n_sorted', 'n_skipped_level', 'n_skipped_id', 'n_zlib', 'n_arrays', 'n_lines')
    assert {k: full[k] for k in keys} == {k: stats[k] for k in keys}
    assert stats['n_spectra'] - stats['n_skipped_id'] == len(objs) and stats['n_lines'] == MC.tags_of(data)
    stats['kept'] = sum(p.n for p in got_packs.values())
    return stats


# ---------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize('n_spectra', [1, 2, 63, 64, 65, 257])
def test_spectrum_counts(n_spectra):
    st = check(MC.plain_file(n_spectra, seed=n_spectra))
    assert st['n_spectra'] == n_spectra and st['n_sorted'] == 0 and st['chunks'] == 1
    assert st['n_zlib'] == st['n_arrays'] == 2 * n_spectra and st['kept'] >= n_spectra


def _with_tags(n_tags, n_spectra, seed):
    """A file of exactly ``n_tags`` tags: padding elements go between the spectra."""
    rng = np.random.default_rng(seed)
    spectra = [MC.spectrum(i, *MC.peaks(rng, 12), charge=2 + i % 2) for i in range(n_spectra)]
    missing = n_tags - MC.tags_of(MC.document(spectra))
    assert missing >= 0
    for k in range(missing):
        spectra[k % n_spectra] += '        <userParam name="pad" value="1"/>\n'
    data = MC.document(spectra)
    assert MC.tags_of(data) == n_tags
    return data


def test_tag_counts_around_the_scan_tile():
    from ann_solo_amd.mzml import SCAN_TILE
    for n_tags in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE, 2 * SCAN_TILE + 1):
        st = check(_with_tags(n_tags, 2, seed=n_tags))
        assert st['n_lines'] == n_tags and st['n_spectra'] == 2


def test_tag_count_beyond_two_scan_levels():
    from ann_solo_amd.mzml import SCAN_TILE
    n_tags = SCAN_TILE * SCAN_TILE + 1                   # block partials of the block partials
    st = check(_with_tags(n_tags, 700, seed=5))
    assert st['n_lines'] == n_tags and st['n_spectra'] == 700


def test_text_lengths_around_the_byte_span():
    """The tag-start pass reads 16 bytes a thread: every length modulo 16, a '<' as the first and the last byte."""
    base = MC.plain_file(2, seed=77).rstrip(b'\n')
    base = base[base.index(b'<indexedmzML'):]            # (blanks may not stand before an XML declaration)
    for pad in range(17):
        assert check(b' ' * pad + base)['n_spectra'] == 2


def _ramp(n):
    return 100.0 + 0.25 * np.arange(n), 1.0 + (np.arange(n) * 7919) % 1000


def test_peak_counts_and_the_size_classes():
    from ann_solo_amd import _lib
    from ann_solo_amd.mzml import MAX_PEAKS, SMALL_PEAKS, read_mzml_packed
    counts = [0, 1, 2, 3, 255, 256, 257, SMALL_PEAKS, SMALL_PEAKS + 1, MAX_PEAKS]
    data = MC.document([MC.spectrum(i, *_ramp(n), f64=(i % 2 == 0, True)) for i, n in enumerate(counts)])
    st = check(data, lenient=True)
    assert st['n_peaks'] == sum(counts) and st['kept'] == len(counts) - 1        # the empty one is dropped
    assert st['n_small'] == 2 * 8
    over = MC.document([MC.spectrum(0, *_ramp(20)), MC.spectrum(1, *_ramp(MAX_PEAKS + 1))])
    with pytest.raises(_lib.AnnSoloMiError) as e:
        read_mzml_packed(over, _cfg(True), DEV)
    assert e.value.code == _lib.ERR_CAPACITY


# ---------------------------------------------------------------------------------------------- encodings
def test_precisions_and_compressions():
    rng = np.random.default_rng(3)
    spectra = []
    for f64 in (True, False):
        for z in (True, False):
            for n in (1, 2, 3, 40, 301):                 # every base64 padding class, with and without zlib
                spectra.append(MC.spectrum(len(spectra), *MC.peaks(rng, n), f64=(f64, f64), z=(z, z)))
    spectra.append(MC.spectrum(len(spectra), *MC.peaks(rng, 33), f64=(True, False), z=(True, False)))   # a mix
    st = check(MC.document(spectra), lenient=True)
    assert st['n_spectra'] == 21 and st['n_zlib'] == 21 and st['n_arrays'] == 42


def _compression_spectra():
    spectra = []
    for name, stream, raw in MC.streams():
        n = len(raw) // 8
        arrays = [MC.array(_ramp(n)[0], 'mz', f64=False, z=False),
                  MC.array(None, 'it', content=base64.b64encode(stream).decode())]
        spectra.append(MC.spectrum(len(spectra), dal=n, arrays=arrays))
    return spectra


def test_compression_cases_as_arrays():
    """The streams of the CPU list (levels, strategies, stored / fixed / dynamic blocks, overlapping and far
    matches, flushes, many blocks) as intensity arrays, beside plain 32-bit m/z."""
    spectra = _compression_spectra()
    st = check(MC.document(spectra), lenient=True)
    assert st['n_spectra'] == len(spectra) >= 24 and st['n_zlib'] == len(spectra)


def test_the_wave_per_array_shape_decodes_the_same(monkeypatch):
    """ASL_MZML_DECODE=wave, the shape profiles/mzml_cost.json compares the default with: the same core, the same
    bytes and the same verdicts."""
    from ann_solo_amd import mzml
    monkeypatch.setenv('ASL_MZML_DECODE', 'wave')
    rng = np.random.default_rng(15)
    mixed = [MC.spectrum(i, *MC.peaks(rng, n), f64=(f64, not f64), z=(z, not z))
             for i, (n, f64, z) in enumerate([(0, True, True), (1, True, False), (2, False, True), (3, False, False),
                                              (301, True, True), (513, False, True), (4096, True, True)])]
    st = check(MC.document(_compression_spectra() + mixed), lenient=True)
    assert st['n_spectra'] >= 31
    good = MC.spectrum(0, *MC.peaks(rng, 12))
    for name in ('a lying defaultArrayLength, too large', 'a lying defaultArrayLength, too small', 'a wrong Adler-32',
                 'a corrupt zlib stream', 'a stray byte in base64', 'padding inside base64'):
        change = dict(DEVIATIONS)[name]
        with pytest.raises(ValueError, match=r'mzML: spectrum 1 '):
            mzml.read_mzml_raw(MC.document([good, MC.spectrum(1, *_pk(), **change)]), DEV)


def test_blanks_inside_base64():
    mz, it = MC.peaks(np.random.default_rng(4), 100)
    text = MC.encode(mz)
    broken = '\n' + '\n'.join(text[i:i + 61] for i in range(0, len(text), 61)) + ' \t\r\n'
    data = MC.document([MC.spectrum(0, mz, it, arrays=[MC.array(mz, 'mz', content=broken), MC.array(it, 'it')])])
    assert check(data)['n_spectra'] == 1


# ---------------------------------------------------------------------------------------------- decoding
def test_descending_mz_is_sorted():
    rng = np.random.default_rng(6)
    mz, it = MC.peaks(rng, 50)
    swapped = mz.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    data = MC.document([MC.spectrum(0, mz[::-1], it), MC.spectrum(1, mz, it), MC.spectrum(2, swapped, it)])
    assert check(data, lenient=True)['n_sorted'] == 2


def test_numerals_at_the_edges_of_the_rule():
    """What asl_mgf_number converts, and what it defers to Python's float()."""
    values = ['500.25', '0500.250', '5.0025e2', '+500.25', '9007199254740993', '1234567890.12345678901', '4.5e-23',
              '1e23', '12345678901234567890e-17', '.5e3', '500.', ' 500.25', '5_00.25']
    rng = np.random.default_rng(9)
    spectra = [MC.spectrum(i, *MC.peaks(rng, 12), rt=v, pmz=v) for i, v in enumerate(values)]
    st = check(MC.document(spectra))
    assert st['n_spectra'] == len(values)
    from ann_solo_amd.mzml import read_mzml_packed
    for bad in ('soon', '1e400', ''):
        with pytest.raises(ValueError, match='spectrum 1 '):
            read_mzml_packed(MC.document([spectra[0], MC.spectrum(1, *MC.peaks(rng, 12), pmz=bad)]), _cfg(), DEV)


def test_other_ms_levels_are_skipped_and_counted():
    rng = np.random.default_rng(10)
    profile = rng.uniform(0.0, 1e6, 98304)               # 1 MB of base64, uncompressed
    spectra = []
    for i in range(7):
        if i in (0, 2, 5):
            spectra.append(MC.spectrum(i, profile, profile, level=1, z=(False, False)))
        elif i == 3:
            spectra.append(MC.spectrum(i, *MC.peaks(rng, 12), level=3))
        else:
            spectra.append(MC.spectrum(i, *MC.peaks(rng, 30)))
    data = MC.document(spectra)
    st = check(data)
    assert st['n_spectra'] == 3 and st['n_skipped_level'] == 4
    from ann_solo_amd.mzml import read_mzml_raw
    assert read_mzml_raw(data, DEV)[3].tolist() == [1, 4, 6]                     # index counts every level
    assert check(data, chunk_bytes=1 << 20)['grown'] > 0                         # an MS1 spectrum fits no chunk


# ---------------------------------------------------------------------------------------------- metadata
def test_charges_precursors_and_identifiers(caplog):
    rng = np.random.default_rng(11)
    pk = lambda: MC.peaks(rng, 20)
    spectra = [MC.spectrum(0, *pk(), charge=None),                               # unknown: entered at 2 and 3
               MC.spectrum(1, *pk(), charge=None, possible=(3,)),
               MC.spectrum(2, *pk(), charge=4, possible=(2, 3)),                 # the charge state goes first
               MC.spectrum(3, *pk(), precursors=2, ions=2, scans=2),             # the first of each
               MC.spectrum(4, *pk(), sid='index=17'),
               MC.spectrum(5, *pk(), sid='sample=1 period=1 cycle=2 experiment=3'),
               MC.spectrum(6, *pk(), sid='scan=12 extra'),
               MC.spectrum(7, *pk(), sid='file=a&amp;b&#32;scan=0041'),
               MC.spectrum(8, *pk(), sid='spectrum=8', rt=None, pmz=None)]           # dropped before its parameters
    with caplog.at_level(logging.WARNING):
        st = check(MC.document(spectra))
    assert st['n_spectra'] == 9 and st['n_skipped_id'] == 3
    assert sum('failed to read spectrum' in r.message for r in caplog.records) >= 6
    from ann_solo_amd.mzml import read_mzml_raw
    raw, rt, ids, index = read_mzml_raw(MC.document(spectra[:8]), DEV)
    assert ids == ['1', '2', '3', '4', '17', '41'] and index.tolist() == [0, 1, 2, 3, 4, 7]
    assert raw.precursor_charge.tolist() == [0, 3, 4, 2, 2, 2] and raw.precursor_mz.tolist() == [500.5] * 6


# ---------------------------------------------------------------------------------------------- layout
def test_layouts():
    rng = np.random.default_rng(12)
    spectra = [MC.spectrum(i, *MC.peaks(rng, 25), charge=(2, 3, None)[i % 3]) for i in range(5)]
    base = check(MC.document(spectra))
    assert base['n_spectra'] == 5                                                # (the chromatogram's array is no peak)
    flat = MC.document(spectra, newlines=False)
    assert b'\n' not in flat and check(flat)['n_peaks'] == base['n_peaks']
    single = MC.document([s.replace('"', "'") for s in spectra])
    assert check(single)['n_peaks'] == base['n_peaks']
    odd = [s.replace('defaultArrayLength=', 'note="a > b" other=\'"\' defaultArrayLength=')
            .replace('name="ms level"', 'name="level > 1"').replace('<binary>', '<binary >') for s in spectra]
    assert check(MC.document(odd))['n_peaks'] == base['n_peaks']
    closed = MC.document(spectra + ['        <spectrum index="5" id="scan=6" defaultArrayLength="0"/>\n',
                                    MC.spectrum(6, *MC.peaks(rng, 25))])
    st = check(closed)
    assert st['n_spectra'] == 6 and st['n_skipped_level'] == 1


_SMALL = ('<spectrum index="%d" id="scan=%d" defaultArrayLength="1"><cvParam accession="MS:1000511" value="2"/>'
          '<scanList><scan><cvParam accession="MS:1000016" value="%d.5"/></scan></scanList><precursorList><precursor>'
          '<selectedIonList><selectedIon><cvParam accession="MS:1000744" value="44%d.5"/></selectedIon>'
          '</selectedIonList></precursor></precursorList><binaryDataArrayList><binaryDataArray>'
          '<cvParam accession="MS:1000521"/><cvParam accession="MS:1000576"/><cvParam accession="MS:1000514"/>'
          '<binary>%s</binary></binaryDataArray><binaryDataArray><cvParam accession="MS:1000521"/>'
          '<cvParam accession="MS:1000576"/><cvParam accession="MS:1000515"/><binary>%s</binary></binaryDataArray>'
          '</binaryDataArrayList></spectrum>')


def test_every_cut_across_one_spectrum():
    """The same result wherever the first chunk ends inside the second of three spectra."""
    from ann_solo_amd import mzml
    one = lambda i: _SMALL % (i, i + 1, i, i, MC.encode([100.5 + i], False, False), MC.encode([7.0 + i], False, False))
    data = ('<mzML><run><spectrumList>' + one(0) + one(1) + one(2) + '</spectrumList></run></mzML>').encode()
    check(data)
    whole = mzml.read_mzml_raw(data, DEV)
    a, b = data.index(b'<spectrum index="1"'), data.index(b'<spectrum index="2"')
    assert b - a < 800
    for cut in range(a - 1, b + 2):
        st = {}
        raw, rt, ids, index = mzml.read_mzml_raw(data, DEV, chunk_bytes=cut, stats=st)
        assert st['chunks'] >= 2
        _same_pack(raw, whole[0])
        assert ids == ['1', '2', '3'] and index.tolist() == [0, 1, 2] and rt.tobytes() == whole[1].tobytes()
    for cut in (1, 50):                                   # chunks that close nothing are doubled
        st = {}
        _same_pack(mzml.read_mzml_raw(data, DEV, chunk_bytes=cut, stats=st)[0], whole[0])
        assert st['grown'] > 0
    check(MC.plain_file(65, seed=65), chunk_bytes=20000)


# ---------------------------------------------------------------------------------------------- errors
def _pk():
    return np.array([100.5, 200.25, 300.125]), np.array([1.0, 2.0, 3.0])


def _arrays(**kw):
    mz, it = _pk()
    return [MC.array(mz, 'mz', **kw), MC.array(it, 'it')]


def _flipped(at):
    stream = bytearray(MC.deflate(_pk()[0].tobytes()))
    stream[at] ^= 0x10
    return base64.b64encode(bytes(stream)).decode()


DEVIATIONS = [
    ('no scan start time', dict(rt=None)),
    ('no selected ion m/z', dict(pmz=None)),
    ('no precursor', dict(precursors=0)),
    ('several possible charges', dict(charge=None, possible=(2, 3))),
    ('a charge with a sign', dict(charge='2+')),
    ('a lying defaultArrayLength, too large', dict(dal=4)),
    ('a lying defaultArrayLength, too small', dict(dal=2)),
    ('no defaultArrayLength', dict(dal='many')),
    ('a param group', dict(head='<referenceableParamGroupRef ref="g"/>')),
    ('a comment', dict(inside='<!-- late -->')),
    ('a CDATA section', dict(inside='<userParam><![CDATA[x]]></userParam>')),
    ('arrayLength', dict(arrays=_arrays(attrs=' arrayLength="3"'))),
    ('integers', dict(arrays=_arrays(precision=MC.cv('1000522', '64-bit integer')))),
    ('no precision', dict(arrays=_arrays(precision=''))),
    ('Numpress', dict(arrays=_arrays(compression=MC.cv('1002312', 'MS-Numpress linear prediction compression')))),
    ('no compression parameter', dict(arrays=_arrays(compression=''))),
    ('no m/z array', dict(arrays=_arrays()[1:])),
    ('a corrupt zlib stream', dict(arrays=_arrays(content=_flipped(6)))),
    ('a wrong Adler-32', dict(arrays=_arrays(content=_flipped(-1)))),
    ('a bad zlib header', dict(arrays=_arrays(content=_flipped(0)))),
    ('a truncated stream', dict(arrays=_arrays(content=base64.b64encode(MC.deflate(_pk()[0].tobytes())[:-3]).decode()))),
    ('a stray byte in base64', dict(arrays=_arrays(content='AAA*'))),
    ('base64 of a bad length', dict(arrays=_arrays(content=MC.encode(_pk()[0])[:-1]))),
    ('padding inside base64', dict(arrays=_arrays(content='AA==' + MC.encode(_pk()[0])))),
    ('an empty compressed array', dict(arrays=_arrays(content=''))),
]


@pytest.mark.parametrize('name, change', DEVIATIONS, ids=[d[0] for d in DEVIATIONS])
def test_deviations_raise_value_errors_that_name_the_spectrum(name, change):
    from ann_solo_amd import mzml
    rng = np.random.default_rng(13)
    good = [MC.spectrum(i, *MC.peaks(rng, 12)) for i in (0, 1, 3)]
    data = MC.document(good[:2] + [MC.spectrum(2, *_pk(), **change)] + good[2:])
    with pytest.raises(ValueError, match='spectrum 2'):
        mzml_ref.read_mzml(data)
    for chunk in (256 << 20, 6000):
        with pytest.raises(ValueError, match=r'mzML: spectrum 2 '):
            mzml.read_mzml_packed(data, _cfg(True), DEV, chunk_bytes=chunk)
    with pytest.raises(ValueError, match=r'mzML: spectrum 2 '):
        mzml.read_mzml_raw(data, DEV)


def test_a_tag_beyond_the_cap_is_an_error_code_not_a_long_walk():
    from ann_solo_amd import _lib, mzml
    mz, it = _pk()
    ok = MC.spectrum(0, mz, it, head='<userParam name="%s"/>' % ('x' * (mzml.MAX_TAG - 20)))
    assert check(MC.document([ok]))['n_spectra'] == 1
    long = MC.spectrum(0, mz, it, head='<userParam name="%s"/>' % ('x' * mzml.MAX_TAG))
    with pytest.raises(_lib.AnnSoloMiError) as e:
        mzml.read_mzml_packed(MC.document([long]), _cfg(), DEV)
    assert e.value.code == _lib.ERR_CAPACITY


def test_an_unclosed_last_spectrum_and_empty_inputs(caplog):
    from ann_solo_amd import mzml
    data = MC.plain_file(3, seed=14)
    cut = data[:data.rindex(b'</spectrum>')]
    with caplog.at_level(logging.WARNING):
        raw, rt, ids, index = mzml.read_mzml_raw(cut, DEV)
    assert ids == ['1', '2'] and any('not closed' in r.message for r in caplog.records)
    for empty in (b'', b'no tag at all', b'<mzML></mzML>', MC.document([])):
        raw, rt, ids, index = mzml.read_mzml_raw(empty, DEV)
        assert raw.n == 0 and ids == [] and len(rt) == 0
        assert mzml.read_mzml_packed(empty, _cfg(), DEV) == ({}, {})


# ---------------------------------------------------------------------------------------------- the search
def _mzml_of(q):
    """The packed queries ``q`` as an mzML file: float64 zlib arrays, the charge stated."""
    o, mz, it = q.offsets.numpy(), q.mz.numpy().astype(np.float64), q.intensity.numpy().astype(np.float64)
    pmz, pz = q.precursor_mz.numpy(), q.precursor_charge.numpy()
    return MC.document([MC.spectrum(i, mz[o[i]:o[i + 1]], it[o[i]:o[i + 1]], pmz=repr(float(pmz[i])),
                                    charge=int(pz[i]), rt='%.3f' % (0.01 * i)) for i in range(q.n)])


def test_search_with_the_switch_is_search_without_it(tmp_path):
    from ann_solo_amd import synthetic
    from ann_solo_amd.library_store import pack_queries
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, aux = synthetic.make_library(3000, seed=41, device='cpu', charges=(2, 3), charge_p=(0.7, 0.3))
    q, _ = synthetic.make_queries(lib, aux, 200, seed=42, open_range=300.0)
    path = tmp_path / 'Queries.mzML'                     # the extension in any letter case
    path.write_bytes(_mzml_of(q))
    kw = dict(num_list=16, num_probe=8, num_candidates=256, index='ivfpq', kmeans_niter=4, batch_size=64)
    tables, called = [], []
    for device_mzml in (True, False):
        def reader(filename):
            assert not device_mzml, 'the switch is on: the query reader must not be called'
            called.append(filename)
            return mzml_ref.read_mzml(filename)
        sl = SpectralLibrary(lib, config=Config.open_search(device_mzml=device_mzml, **kw), device=DEV,
                             query_reader=reader)
        lmeta = {z: [dict(identifier=int(r), peptide=f'P{r}K', precursor_mz=float(p), is_decoy=False)
                     for r, p in enumerate(part.precursor_mz)] for z, part in sl.partitions.items()}
        t = sl.search(str(path), library_meta=lmeta)
        tables.append((t, [(s.query_identifier, s.query_index, s.retention_time) for s in t]))
        if not device_mzml:      # and the switch off is the path as it was: the packed driver over pack_queries
            qs, qm = pack_queries(mzml_ref.read_mzml(str(path)), sl.config, DEV)
            tables.append((sl.search(qs, qm, lmeta), None))
        sl.shutdown()
    assert called == [str(path)]                         # off: the .mzML name went to query_reader as before
    (on, on_ids), (off, off_ids), (packed, _) = tables
    assert len(on) > 100 and on_ids == off_ids
    for t in (off, packed):
        for col in ('charge', 'qrow', 'lib_row', 'score', 'q'):
            a, b = np.asarray(getattr(on, col)), np.asarray(getattr(t, col))
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), col
