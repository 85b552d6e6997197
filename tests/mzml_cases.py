"""Generators of the mzML reader's test inputs (tests/test_mzml_cpu.py, tests/test_gpu_mzml.py, scripts/mzml_cost.py).

No converter-written mzML exists where this project is tested, so the files are generated here in the layout the
converters (msconvert, ThermoRawFileParser) write: an ``indexedmzML`` wrapper, ``cvList``, ``run``, ``spectrumList``,
a ``chromatogramList`` with a binary array of its own, ``indexList``. Arrays are compressed with Python's ``zlib``.
"""
import base64
import re
import struct
import zlib

import numpy as np

HEAD = '''<?xml version="1.0" encoding="utf-8"?>
<indexedmzML xmlns="http://psi.hupo.org/ms/mzml" xmlns:xsi="http://www.w3.org/2001/XMLSchema-instance">
  <mzML xmlns="http://psi.hupo.org/ms/mzml" id="generated" version="1.1.0">
    <cvList count="2">
      <cv id="MS" fullName="Proteomics Standards Initiative Mass Spectrometry Ontology" version="4.1.30"/>
      <cv id="UO" fullName="Unit Ontology" version="09:04:2014"/>
    </cvList>
    <fileDescription>
      <fileContent>
        <cvParam cvRef="MS" accession="MS:1000580" name="MSn spectrum" value=""/>
        <cvParam cvRef="MS" accession="MS:1000511" name="ms level" value="2"/>
      </fileContent>
    </fileDescription>
    <!-- a comment before the first spectrum is legal -->
    <softwareList count="1">
      <software id="generator" version="1.0">
        <cvParam cvRef="MS" accession="MS:1000799" name="custom unreleased software tool" value="mzml_cases"/>
      </software>
    </softwareList>
    <dataProcessingList count="1">
      <dataProcessing id="dp">
        <processingMethod order="0" softwareRef="generator">
          <cvParam cvRef="MS" accession="MS:1000544" name="Conversion to mzML" value=""/>
        </processingMethod>
      </dataProcessing>
    </dataProcessingList>
    <run id="run" defaultInstrumentConfigurationRef="IC1">
      <spectrumList count="%d" defaultDataProcessingRef="dp">
'''
TAIL = '''      </spectrumList>
      <chromatogramList count="1" defaultDataProcessingRef="dp">
        <chromatogram index="0" id="TIC" defaultArrayLength="3">
          <cvParam cvRef="MS" accession="MS:1000235" name="total ion current chromatogram" value=""/>
          <precursor>
            <isolationWindow>
              <cvParam cvRef="MS" accession="MS:1000827" name="isolation window target m/z" value="1.0"/>
            </isolationWindow>
          </precursor>
          <binaryDataArrayList count="1">
            <binaryDataArray encodedLength="32">
              <cvParam cvRef="MS" accession="MS:1000523" name="64-bit float" value=""/>
              <cvParam cvRef="MS" accession="MS:1000576" name="no compression" value=""/>
              <cvParam cvRef="MS" accession="MS:1000515" name="intensity array" value=""/>
              <binary>AAAAAAAA8D8AAAAAAAAAQAAAAAAAAAhA</binary>
            </binaryDataArray>
          </binaryDataArrayList>
        </chromatogram>
      </chromatogramList>
    </run>
  </mzML>
  <indexList count="1">
    <index name="spectrum">
      <offset idRef="none">0</offset>
    </index>
  </indexList>
  <indexListOffset>0</indexListOffset>
</indexedmzML>
'''


def encode(values, f64=True, z=True, level=6, strategy=zlib.Z_DEFAULT_STRATEGY) -> str:
    raw = np.asarray(values, np.float64 if f64 else np.float32).tobytes()
    if z:
        c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
        raw = c.compress(raw) + c.flush()
    return base64.b64encode(raw).decode()


def cv(acc, name, value='', q='"', more=''):
    return f'<cvParam cvRef={q}MS{q} accession={q}MS:{acc}{q} name={q}{name}{q} value={q}{value}{q}{more}/>'


def array(values, kind, f64=True, z=True, q='"', content=None, attrs='', precision=None, compression=None, **kw):
    """One ``<binaryDataArray>``; ``content`` overrides the encoded text, ``precision`` / ``compression`` the
    cvParam lines."""
    text = encode(values, f64, z, **kw) if content is None else content
    prec = precision if precision is not None else \
        (cv('1000523', '64-bit float', q=q) if f64 else cv('1000521', '32-bit float', q=q))
    comp = compression if compression is not None else \
        (cv('1000574', 'zlib compression', q=q) if z else cv('1000576', 'no compression', q=q))
    what = cv('1000514', 'm/z array', q=q, more=f' unitCvRef={q}MS{q} unitAccession={q}MS:1000040{q}') \
        if kind == 'mz' else cv('1000515', 'intensity array', q=q) if kind == 'it' else \
        cv('1000786', 'non-standard data array', 'noise', q=q)
    return (f'          <binaryDataArray encodedLength={q}{len(text)}{q}{attrs}>\n            {prec}\n'
            f'            {comp}\n            {what}\n            <binary>{text}</binary>\n'
            f'          </binaryDataArray>\n')


def spectrum(index, mz=(), it=(), sid=None, level=2, f64=(True, True), z=(True, True), rt='1.5', pmz='500.5',
             charge=2, possible=(), dal=None, q='"', arrays=None, head='', scans=1, precursors=1, ions=1,
             inside='', **kw):
    """One ``<spectrum>`` element. ``charge`` None: unknown; ``possible``: MS:1000633 values; ``arrays``: the
    ``<binaryDataArray>`` elements ready-made; ``head`` / ``inside``: text put after the opening tag / before the
    closing one; ``rt`` / ``pmz`` None: the parameter is left out."""
    sid = f'controllerType=0 controllerNumber=1 scan={index + 1}' if sid is None else sid
    n = len(mz) if dal is None else dal
    out = [f'        <spectrum index={q}{index}{q} id={q}{sid}{q} defaultArrayLength={q}{n}{q}>\n{head}',
           f'          {cv("1000511", "ms level", level, q)}\n',
           f'          {cv("1000580", "MSn spectrum", q=q)}\n',
           f'          {cv("1000127", "centroid spectrum", q=q)}\n',
           f'          <scanList count={q}{scans}{q}>\n            {cv("1000795", "no combination", q=q)}\n']
    for k in range(scans):
        out.append(f'            <scan>\n')
        if rt is not None:
            unit = f' unitCvRef={q}UO{q} unitAccession={q}UO:0000031{q} unitName={q}minute{q}'
            out.append(f'              {cv("1000016", "scan start time", rt if k == 0 else "99.0", q, unit)}\n')
        out.append(f'              <scanWindowList count={q}1{q}><scanWindow>'
                   f'{cv("1000501", "scan window lower limit", "100", q)}</scanWindow></scanWindowList>\n'
                   f'            </scan>\n')
    out.append('          </scanList>\n')
    if level != 1 and precursors:
        out.append(f'          <precursorList count={q}{precursors}{q}>\n')
        for k in range(precursors):
            out.append(f'            <precursor spectrumRef={q}scan=1{q}>\n              <isolationWindow>\n'
                       f'                {cv("1000827", "isolation window target m/z", "1.25", q)}\n'
                       f'              </isolationWindow>\n              <selectedIonList count={q}{ions}{q}>\n')
            for j in range(ions):
                first = k == 0 and j == 0
                out.append('                <selectedIon>\n')
                if pmz is not None or not first:
                    out.append(f'                  {cv("1000744", "selected ion m/z", pmz if first else "77.5", q)}\n')
                if not first:
                    out.append(f'                  {cv("1000041", "charge state", 7, q)}\n')
                elif charge is not None:
                    out.append(f'                  {cv("1000041", "charge state", charge, q)}\n')
                if first:
                    for p in possible:
                        out.append(f'                  {cv("1000633", "possible charge state", p, q)}\n')
                out.append(f'                  {cv("1000042", "peak intensity", "1e5", q)}\n'
                           '                </selectedIon>\n')
            out.append(f'              </selectedIonList>\n              <activation>\n'
                       f'                {cv("1000422", "beam-type collision-induced dissociation", q=q)}\n'
                       f'              </activation>\n            </precursor>\n')
        out.append('          </precursorList>\n')
    if arrays is None:
        arrays = [array(mz, 'mz', f64[0], z[0], q, **kw), array(it, 'it', f64[1], z[1], q, **kw)]
    out.append(f'          <binaryDataArrayList count={q}{len(arrays)}{q}>\n{"".join(arrays)}'
               f'          </binaryDataArrayList>\n{inside}        </spectrum>\n')
    return ''.join(out)


def document(spectra, newlines=True) -> bytes:
    data = (HEAD % len(spectra) + ''.join(spectra) + TAIL).encode()
    return data if newlines else re.sub(rb'>\s+<', b'><', data).replace(b'\n', b' ')


def peaks(rng, n, lo=150.0, hi=1400.0):
    """n ascending m/z (to 4 decimals, exact in neither float format) and intensities."""
    mz = np.sort(np.round(rng.uniform(lo, hi, n), 4))
    return mz, np.round(rng.uniform(1.0, 1e4, n), 1)


def plain_file(n_spectra, seed=0, n_peaks=24, **kw) -> bytes:
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_spectra):
        mz, it = peaks(rng, n_peaks)
        out.append(spectrum(i, mz, it, rt='%.4f' % (0.5 + 0.01 * i), pmz='%.4f' % rng.uniform(300, 900),
                            charge=(2, 3, None)[i % 3], **kw))
    return document(out)


def tags_of(data: bytes) -> int:
    return data.count(b'<')


# ---------------------------------------------------------------------------------------------- decoder streams
def deflate(raw: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return c.compress(raw) + c.flush()


def named_arrays():
    """(name, raw bytes) of the compression cases: what the CPU test feeds the decoder and the GPU test reads as
    arrays (each a whole number of float64)."""
    rng = np.random.default_rng(7)
    noise = rng.uniform(100.0, 2000.0, 4096).astype(np.float64).tobytes()
    return [('constant', np.full(4096, 445.12).tobytes()),          # distance 8, length 258: overlapping copies
            ('noise', noise), ('ramp', np.arange(300, dtype=np.float64).tobytes())]


def far_stream():
    """(zlib stream, raw bytes): 4096 float64 whose last value repeats the first, written by hand as a stored block
    of 32 760 bytes and a fixed block with one match of length 8 at distance 32 760 (zlib itself never looks back
    further than 32 506)."""
    head = np.random.default_rng(8).uniform(1.0, 1e4, 4095).tobytes()
    bits = []

    def put(value, n, msb_first=False):
        order = range(n - 1, -1, -1) if msb_first else range(n)
        bits.extend((value >> k) & 1 for k in order)
    put(1, 1), put(1, 2)                                            # BFINAL, fixed codes
    put(262 - 256, 7, True)                                         # length 8
    put(29, 5, True), put(32760 - 24577, 13)                        # distance code 29 and its 13 extra bits
    put(0, 7, True)                                                 # end of block
    bits.extend([0] * (-len(bits) % 8))
    tail = bytes(sum(b << k for k, b in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8))
    raw = head + head[:8]
    stream = b'\x78\x01' + b'\x00' + struct.pack('<HH', len(head), len(head) ^ 0xffff) + head + tail + \
        struct.pack('>I', zlib.adler32(raw))
    assert zlib.decompress(stream) == raw
    return stream, raw


def streams():
    """(name, zlib stream, raw bytes) over the levels, strategies and block structures of the issue's list."""
    out = []
    for name, raw in named_arrays():
        for level in (0, 1, 6, 9):
            out.append((f'{name}-l{level}', deflate(raw, level), raw))
        for sname, s in (('fixed', zlib.Z_FIXED), ('huffman', zlib.Z_HUFFMAN_ONLY), ('rle', zlib.Z_RLE)):
            out.append((f'{name}-{sname}', deflate(raw, 6, s), raw))
    raw = named_arrays()[1][1]
    c = zlib.compressobj(6)
    flushed = c.compress(raw[:8000]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(raw[8000:16000]) + \
        c.flush(zlib.Z_FULL_FLUSH) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(raw[16000:]) + c.flush()
    out.append(('full-flush', flushed, raw))                        # empty stored blocks inside
    c = zlib.compressobj(1, zlib.DEFLATED, 9, 1)                    # small window and memLevel: many blocks
    out.append(('multi-block', c.compress(raw) + c.flush(), raw))
    out.append(('far',) + far_stream())
    return out


def mutations(stream: bytes):
    """Every truncation and every single-bit flip of ``stream``."""
    for k in range(len(stream)):
        yield stream[:k]
    for k in range(len(stream)):
        for b in range(8):
            yield stream[:k] + bytes([stream[k] ^ (1 << b)]) + stream[k + 1:]


def small_streams():
    raw = np.array([301.25, 1.0, 777.0625, 301.25], np.float64).tobytes() + b'abcabcabcabc' * 3
    skewed = np.random.default_rng(3).choice(np.frombuffer(b'aaaaaaaabbbbccde\x00\x01', np.uint8), 200).tobytes()
    return [('stored', deflate(raw, 0)), ('dynamic', deflate(skewed, 9))]


def python_verdict(stream: bytes):
    """zlib.decompress's: the bytes, or None for an exception."""
    try:
        return zlib.decompress(stream)
    except zlib.error:
        return None


def corpus_record(b64: bytes, use_zlib: bool, cap: int, want) -> bytes:
    """One record of tests/native/inflate_check.cpp's corpus; ``want``: the bytes, or None for an error."""
    w = b'' if want is None else want
    return struct.pack('<BBIII', int(use_zlib), int(want is None), len(b64), cap, len(w)) + b64 + w
