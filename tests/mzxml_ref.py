"""The mzXML dialect of ``ann_solo_amd.mzxml`` restated in plain Python: the definition the device reader is tested
against (include/annsolo_mi.h "mzXML query files", DESIGN.md 3 "Query files").

The rules are what the reference's ``read_mzxml`` / ``_parse_spectrum_mzxml`` (reader.py:742-811) read through
pyteomics' ``mzxml.MzXML``, written down from its documented behaviour with ``xml.etree.ElementTree``, ``base64``,
``zlib`` and numpy. pyteomics is not a dependency of this project, so the restatement is unpinned and IS the
definition. Where the reference crashes (``KeyError``, ``TypeError``, ``zlib.error``, ``binascii.Error``) the
restatement raises ``ValueError`` naming the scan by its ``index``; the one ``ValueError`` the reference catches -- a
``num`` that ``int()`` refuses -- drops the scan with a warning here too.

``read_mzxml(source)`` takes a path or bytes and returns the list of spectrum objects ``pack_queries`` takes (with
``nested``: the scan lies inside another scan's element).
"""
import base64
import logging
import math
import os
import re
import zlib
from types import SimpleNamespace
import xml.etree.ElementTree as ET

import numpy as np

MAX_PEAKS = 4096
_B64 = re.compile(rb'[A-Za-z0-9+/]*={0,2}')
_BLANKS = bytes([9, 10, 11, 12, 13, 32])
_DIGITS = re.compile(r'[0-9]+')
_SCAN = re.compile(rb'<scan[\s>/]')
_NUM = r'(\d+\.?\d*)'
_DURATION = re.compile(rf'P(?:\d+\.?\d*Y)?(?:\d+\.?\d*M)?(?:\d+\.?\d*D)?(?:T(?:{_NUM}H)?(?:{_NUM}M)?(?:{_NUM}S)?)?')


def _local(e):
    return e.tag.rsplit('}', 1)[-1]


def _number(value, where, what):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f'{where}: {what} {value!r} is not a number') from None
    if not math.isfinite(v):
        raise ValueError(f'{where}: non-finite {what} {value!r}')
    return v


def duration_minutes(value: str, where: str = 'retentionTime') -> float:
    """pyteomics' rule for ``xs:duration``: a value that does not begin with ``P`` is the numeral as written; else
    ``minutes + hours * 60.0 + seconds / 60.0`` in that order, years, months and days ignored."""
    if not value.startswith('P'):
        return _number(value, where, 'retentionTime')
    m = _DURATION.fullmatch(value)
    if m is None or value == 'P' or value.endswith('T'):
        raise ValueError(f'{where}: retentionTime {value!r} is not a duration')
    hours, minutes, seconds = (float(g) if g else 0.0 for g in m.groups())
    v = minutes + hours * 60.0 + seconds / 60.0
    if not math.isfinite(v):
        raise ValueError(f'{where}: non-finite retentionTime {value!r}')
    return v


def decode(text: bytes, use_zlib: bool, expect: int, where: str) -> bytes:
    """The content of one ``<peaks>``: exactly ``expect`` bytes, or ``ValueError``."""
    chars = text.translate(None, _BLANKS)
    if len(chars) % 4 or not _B64.fullmatch(chars):
        raise ValueError(f'{where}: not base64')
    raw = base64.b64decode(chars)
    if use_zlib and not (expect == 0 and not raw):      # (an empty spectrum may have no characters at all)
        if len(raw) > expect + expect // 8 + 64:
            raise ValueError(f'{where}: a compressed stream longer than the peaks allow')
        try:
            d = zlib.decompressobj()
            raw = d.decompress(raw, expect + 1)         # (never more than one byte beyond the peaks)
            if not d.eof and len(raw) <= expect:
                raise zlib.error('incomplete or truncated stream')
        except zlib.error as e:
            raise ValueError(f'{where}: {e}') from None
    if len(raw) != expect:
        raise ValueError(f'{where}: {len(raw)} bytes, peaksCount promises {expect}')
    return raw


def read_mzxml(source):
    if isinstance(source, (str, os.PathLike)):
        with open(source, 'rb') as f:
            data = f.read()
    else:
        data = bytes(source)
    first = _SCAN.search(data)
    if first is not None:
        marks = [p for p in (data.find(b'<!--', first.start()), data.find(b'<![CDATA[', first.start())) if p >= 0]
        if marks:
            k = len(_SCAN.findall(data, 0, min(marks)))
            raise ValueError(f'scan {k - 1}: a comment or CDATA section after the first <scan')
    if not data.strip():
        return []
    try:
        root = ET.fromstring(data)
    except ET.ParseError as e:
        raise ValueError(f'not well-formed: {e}') from None
    parent = {c: p for p in root.iter() for c in p}
    # document order: every <scan> gets its index; what a scan owns lies in its head, before its first child scan
    scans, heads, n_seen = [], {}, 0
    for e in root.iter():
        name = _local(e)
        if name == 'scan':
            scans.append(e)
            n_seen += 1
            kids = list(e)
            stop = next((k for k, c in enumerate(kids) if _local(c) == 'scan'), len(kids))
            heads[e] = kids[:stop]
        elif name in ('precursorMz', 'peaks'):
            p = parent.get(e)
            if p is None or _local(p) != 'scan' or not any(e is h for h in heads[p]):
                raise ValueError(f'scan {n_seen - 1}: a <{name}> outside any scan')
    for index, sc in enumerate(scans):
        level = sc.get('msLevel')
        if level is not None and not _DIGITS.fullmatch(level):
            raise ValueError(f'scan {index}: msLevel {level!r} is not a number')
    out = []
    for index, sc in enumerate(scans):
        level = sc.get('msLevel')
        if level is None or int(level) != 2:
            continue
        where = f'scan {index}'
        head = heads[sc]
        # what fails while pyteomics iterates over the file
        n = sc.get('peaksCount')
        if n is None or not _DIGITS.fullmatch(n):
            raise ValueError(f'{where}: peaksCount {n!r}')
        n = int(n)
        if n > MAX_PEAKS:
            raise OverflowError(f'{where}: more than {MAX_PEAKS} peaks')
        peaks = [c for c in head if _local(c) == 'peaks']
        if not peaks:
            raise ValueError(f'{where}: no <peaks>')
        if len(peaks) > 1:
            raise ValueError(f'{where}: more than one <peaks>')
        pk = peaks[0]
        if pk.get('precision') not in ('32', '64'):
            raise ValueError(f'{where}: a missing or unsupported precision {pk.get("precision")!r}')
        if pk.get('byteOrder', 'network') != 'network':
            raise ValueError(f'{where}: byteOrder {pk.get("byteOrder")!r}')
        if pk.get('contentType', 'm/z-int') != 'm/z-int' or pk.get('pairOrder', 'm/z-int') != 'm/z-int':
            raise ValueError(f'{where}: a contentType or pairOrder other than m/z-int')
        if pk.get('compressionType', 'none') not in ('none', 'zlib'):
            raise ValueError(f'{where}: compressionType {pk.get("compressionType")!r}')
        width = int(pk.get('precision')) // 8
        raw = decode((pk.text or '').encode('ascii', 'replace'), pk.get('compressionType') == 'zlib', n * 2 * width,
                     where)
        pairs = np.frombuffer(raw, f'>f{width}').astype(f'=f{width}')
        if sc.get('num') is None:
            raise ValueError(f'{where}: no num')
        # the reference's parser: the identifier first
        try:
            identifier = str(int(sc.get('num')))
        except ValueError:
            logging.warning('mzXML: failed to read scan %s: its num is not an integer', sc.get('num'))
            continue
        if sc.get('retentionTime') is None:
            raise ValueError(f'{where}: no retentionTime')
        rt = duration_minutes(sc.get('retentionTime'), where)
        precursors = [c for c in head if _local(c) == 'precursorMz']
        if not precursors:
            raise ValueError(f'{where}: no <precursorMz>')
        pmz = _number((precursors[0].text or '').strip(), where, 'precursor m/z')
        z = precursors[0].get('precursorCharge')
        if z is not None:
            if not _DIGITS.fullmatch(z) or not 1 <= int(z) <= 255:
                raise ValueError(f'{where}: precursorCharge {z!r} is not a number in 1 .. 255')
            z = int(z)
        up = parent.get(sc)
        out.append(SimpleNamespace(identifier=identifier, precursor_mz=pmz, precursor_charge=z, mz=pairs[0::2],
                                   intensity=pairs[1::2], retention_time=rt, index=index,
                                   nested=up is not None and _local(up) == 'scan'))
    return out
