"""Generators of the mzXML reader's test inputs (tests/test_mzxml_cpu.py, tests/test_gpu_mzxml.py,
scripts/mzxml_cost.py).

No converter-written mzXML exists where this project is tested, so the files are generated here in the layouts the
converters write: ReAdW-style nesting (an MS1 ``<scan>`` holds its MS2 scans, an MS2 its MS3) and msconvert-style
flat files; ``msRun`` with ``parentFile``, ``msInstrument`` and a ``dataProcessing`` that holds the schema's
``<comment>`` element; a trailing ``<index>`` / ``<offset>`` / ``<indexOffset>`` / ``<sha1>`` block; the mzXML 2.x
``pairOrder`` attribute in place of ``contentType``; a self-closing ``<peaks/>``. Streams are compressed with
Python's ``zlib``.
"""
import base64
import re
import struct
import zlib

import numpy as np

from mzml_cases import deflate, peaks, tags_of  # noqa: F401  (shared with the mzML generator)

HEAD = '''<?xml version="1.0" encoding="ISO-8859-1"?>
<mzXML xmlns="http://sashimi.sourceforge.net/schema_revision/mzXML_3.2"
       xmlns:xsi="http://www.w3.org/2001/XMLSchema-instance"
       xsi:schemaLocation="http://sashimi.sourceforge.net/schema_revision/mzXML_3.2 mzXML_idx_3.2.xsd">
  <!-- a comment before the first scan is legal -->
  <msRun scanCount="%d" startTime="PT0.5S" endTime="PT3600S">
    <parentFile fileName="generated.raw" fileType="RAWData" fileSha1="0000000000000000000000000000000000000000"/>
    <msInstrument msInstrumentID="1">
      <msManufacturer category="msManufacturer" value="generated"/>
      <msModel category="msModel" value="mzxml_cases"/>
      <software type="acquisition" name="none" version="1.0"/>
    </msInstrument>
    <dataProcessing centroided="1">
      <software type="conversion" name="mzxml_cases" version="1.0"/>
      <comment>peaks &lt; 10 are kept; the schema's comment element is an ordinary tag</comment>
    </dataProcessing>
'''
TAIL = '''  </msRun>
'''
INDEX = '''  <index name="scan">
    <offset id="1">1268</offset>
    <offset id="2">2761</offset>
  </index>
  <indexOffset>4242</indexOffset>
  <sha1>da39a3ee5e6b4b0d3255bfef95601890afd80709</sha1>
'''


def pairs_bytes(mz, it, f64=False) -> bytes:
    """The interleaved big-endian (m/z, intensity) pairs."""
    a = np.empty(2 * len(mz), '>f8' if f64 else '>f4')
    with np.errstate(over='ignore'):
        a[0::2], a[1::2] = mz, it
    return a.tobytes()


def encode(mz, it, f64=False, z=False, zlevel=6) -> str:
    raw = pairs_bytes(mz, it, f64)
    return base64.b64encode(deflate(raw, zlevel) if z else raw).decode()


def peaks_tag(mz=(), it=(), f64=False, z=False, q='"', content=None, precision=None, order='contentType',
              order_value='m/z-int', byte_order='network', compression=None, self_closing=False, attrs='', zlevel=6):
    """One ``<peaks>`` element; ``content`` overrides the encoded text; ``order``: the attribute that names the
    pairs (``contentType``, mzXML 2.x ``pairOrder``, or None); ``compression``: the attribute's value (default:
    ``zlib`` / ``none`` by ``z``; ``''`` leaves the attribute out); ``zlevel``: zlib's level."""
    text = encode(mz, it, f64, z, zlevel) if content is None else content
    precision = ('64' if f64 else '32') if precision is None else precision
    compression = ('zlib' if z else 'none') if compression is None else compression
    a = [] if precision == '' else [f'precision={q}{precision}{q}']
    if byte_order is not None:
        a.append(f'byteOrder={q}{byte_order}{q}')
    if order is not None:
        a.append(f'{order}={q}{order_value}{q}')
    if compression != '':
        a += [f'compressionType={q}{compression}{q}', f'compressedLen={q}{len(text) if z else 0}{q}']
    head = '<peaks ' + '\n             '.join(a) + attrs
    return head + '/>' if self_closing else f'{head}>{text}</peaks>'


def scan(num, mz=(), it=(), level=2, f64=False, z=False, rt='PT1.5S', pmz='500.5', charge=2, count=None, q='"',
         peaks_xml=None, head='', inside='', children=(), attrs='', pad='    ', precursor_attrs='', **kw):
    """One ``<scan>`` element with its child scans inside. ``level`` None: no msLevel; ``charge`` None: no
    precursorCharge; ``rt`` / ``pmz`` None: the attribute / the element is left out; ``count``: peaksCount where it
    is not the number of peaks (False: no attribute); ``peaks_xml``: the ``<peaks>`` element(s) ready-made; ``head`` / ``inside``: text
    put after the opening tag / before the closing one."""
    n = len(mz) if count is None else count
    a = [f'num={q}{num}{q}']
    if level is not None:
        a.append(f'msLevel={q}{level}{q}')
    if n is not False:
        a.append(f'peaksCount={q}{n}{q}')
    a.append(f'polarity={q}+{q} scanType={q}Full{q}')
    if rt is not None:
        a.append(f'retentionTime={q}{rt}{q}')
    a.append(f'lowMz={q}100{q} highMz={q}2000{q} basePeakMz={q}445.12{q} basePeakIntensity={q}1e5{q}'
             f' totIonCurrent={q}1e6{q}{attrs}')
    out = [f'{pad}<scan ' + f'\n{pad}      '.join(a) + f'>\n{head}']
    if level != 1 and pmz is not None:
        z_attr = '' if charge is None else f' precursorCharge={q}{charge}{q}'
        out.append(f'{pad}  <precursorMz precursorIntensity={q}1234.5{q}{z_attr} activationMethod={q}CID{q}'
                   f'{precursor_attrs}>{pmz}</precursorMz>\n')
    out.append(f'{pad}  {peaks_tag(mz, it, f64, z, q, **kw) if peaks_xml is None else peaks_xml}\n')
    for c in children:
        out.append(c)
    out.append(f'{inside}{pad}</scan>\n')
    return ''.join(out)


def document(scans, index=True, newlines=True) -> bytes:
    n = sum(len(re.findall(r'<scan[\s>/]', s)) for s in scans)
    data = (HEAD % n + ''.join(scans) + TAIL + (INDEX if index else '') + '</mzXML>\n').encode()
    return data if newlines else re.sub(rb'>\s+<', b'><', data).replace(b'\n', b' ')


def nested_file(n_groups, per_group=2, seed=0, n_peaks=24, ms1_peaks=200, ms3=False, **kw) -> bytes:
    """ReAdW-style: ``n_groups`` MS1 scans, each holding ``per_group`` MS2 scans (and, with ``ms3``, each of these one
    MS3 scan)."""
    rng = np.random.default_rng(seed)
    out, num = [], 1
    for g in range(n_groups):
        survey = num
        num += 1
        kids = []
        for k in range(per_group):
            mz, it = peaks(rng, n_peaks)
            mine = num
            num += 1
            sub = []
            if ms3:
                sub = [scan(num, *peaks(rng, 5), level=3, pad='        ', rt='PT%.3fS' % (60.0 + num))]
                num += 1
            kids.append(scan(mine, mz, it, rt='PT%.4fS' % (30.0 + 0.61 * mine), pmz='%.4f' % rng.uniform(300, 900),
                             charge=(2, 3, None)[mine % 3], pad='      ', children=sub, **kw))
        out.append(scan(survey, *peaks(rng, ms1_peaks), level=1, rt='PT%.4fS' % (30.0 + 0.61 * survey),
                        children=kids, f64=kw.get('f64', False), z=kw.get('z', False)))
    return document(out)


def flat_file(n_scans, seed=0, n_peaks=24, every=0, **kw) -> bytes:
    """msconvert-style: every scan at top level; with ``every`` > 0 an MS1 scan before each group of that many."""
    rng = np.random.default_rng(seed)
    out, num = [], 1
    for i in range(n_scans):
        if every and i % every == 0:
            out.append(scan(num, *peaks(rng, 50), level=1, rt='PT%dS' % num))
            num += 1
        mz, it = peaks(rng, n_peaks)
        out.append(scan(num, mz, it, rt='PT%.4fS' % (0.5 + 0.61 * num), pmz='%.4f' % rng.uniform(300, 900),
                        charge=(2, 3, None)[num % 3], **kw))
        num += 1
    return document(out)


def far_stream():
    """(zlib stream, raw bytes) of 64 KiB -- 4096 pairs of float64 -- written by hand: two stored blocks of 32 768
    bytes, then a fixed block with one match of length 8 at distance 32 768, DEFLATE's largest, that reaches from the
    last pair back into the first half of the window; the raw bytes are 65 544 less the match: the stored blocks
    hold 65 528 bytes."""
    rng = np.random.default_rng(8)
    mz = np.sort(np.round(rng.uniform(150.0, 1400.0, 4096), 4))
    it = np.round(rng.uniform(1.0, 1e4, 4096), 1)
    raw = bytearray(pairs_bytes(mz, it, True))
    assert len(raw) == 65536
    raw[-8:] = raw[-8 - 32768:-32768]                   # the last value repeats the one 32 768 bytes before it
    raw = bytes(raw)
    bits = []

    def put(value, n, msb_first=False):
        order = range(n - 1, -1, -1) if msb_first else range(n)
        bits.extend((value >> k) & 1 for k in order)
    put(1, 1), put(1, 2)                                # BFINAL, fixed codes
    put(262 - 256, 7, True)                             # length 8
    put(29, 5, True), put(32768 - 24577, 13)            # distance code 29 and its 13 extra bits
    put(0, 7, True)                                     # end of block
    bits.extend([0] * (-len(bits) % 8))
    tail = bytes(sum(b << k for k, b in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8))
    stored = b''
    body = raw[:-8]
    for a in range(0, len(body), 32768):
        part = body[a:a + 32768]
        stored += b'\x00' + struct.pack('<HH', len(part), len(part) ^ 0xffff) + part
    stream = b'\x78\x01' + stored + tail + struct.pack('>I', zlib.adler32(raw))
    assert zlib.decompress(stream) == raw
    back = np.frombuffer(raw, '>f8')
    return stream, raw, back[0::2].astype(np.float64), back[1::2].astype(np.float64)
