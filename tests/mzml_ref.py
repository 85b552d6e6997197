"""The mzML dialect of ``ann_solo_amd.mzml`` restated in plain Python: the definition the device reader is tested
against (include/annsolo_mi.h "mzML query files", DESIGN.md 3 "Query files").

The rules are what the reference's ``read_mzml`` / ``_parse_spectrum_mzml`` (reader.py:659-740) read through
pyteomics' ``mzml.MzML``, written down from its documented behaviour with ``xml.etree.ElementTree``, ``base64`` and
``zlib``. pyteomics is not a dependency of this project, so the restatement is unpinned and IS the definition. Where
the reference crashes (``KeyError``, ``TypeError``, ``zlib.error``, ``binascii.Error``) the restatement raises
``ValueError`` naming the spectrum by its ``index``; the one ``ValueError`` the reference catches -- an id without a
scan or index number -- drops the spectrum with a warning here too.

``read_mzml(source)`` takes a path or bytes and returns the list of spectrum objects ``pack_queries`` takes.
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
_SPECTRUM = re.compile(rb'<spectrum[\s>/]')
_PRECISION = {'MS:1000523': '<f8', 'MS:1000521': '<f4'}
_BAD_PRECISION = {'MS:1000519', 'MS:1000522', 'MS:1000520', 'MS:1001479'}
_COMPRESSION = {'MS:1000576': False, 'MS:1000574': True}
_BAD_COMPRESSION = {'MS:1002312', 'MS:1002313', 'MS:1002314', 'MS:1002746', 'MS:1002747', 'MS:1002748',
                    'MS:1003089', 'MS:1003090'}


def _local(e):
    return e.tag.rsplit('}', 1)[-1]


def _children(e, name):
    return [c for c in e if _local(c) == name]


def _descendants(e, name):
    return [c for c in e.iter() if _local(c) == name and c is not e]


def _params(e, accessions):
    """The direct cvParam children of ``e`` with one of ``accessions``, in order."""
    return [c for c in _children(e, 'cvParam') if c.get('accession') in accessions]


def _number(value, where, what):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f'{where}: {what} {value!r} is not a number') from None
    if not math.isfinite(v):
        raise ValueError(f'{where}: non-finite {what} {value!r}')
    return v


def _charge(value, where):
    if value is None or not _DIGITS.fullmatch(value) or not 1 <= int(value) <= 255:
        raise ValueError(f'{where}: charge {value!r} is not a number in 1 .. 255')
    return int(value)


def decode(text: bytes, use_zlib: bool, expect: int, where: str) -> bytes:
    """The content of one ``<binary>``: exactly ``expect`` bytes, or ``ValueError``."""
    chars = text.translate(None, _BLANKS)
    if len(chars) % 4 or not _B64.fullmatch(chars):
        raise ValueError(f'{where}: not base64')
    raw = base64.b64decode(chars)
    if use_zlib:
        if len(raw) > expect + expect // 8 + 64:
            raise ValueError(f'{where}: a compressed stream longer than the array allows')
        try:
            d = zlib.decompressobj()
            raw = d.decompress(raw, expect + 1)         # (never more than one byte beyond the array)
            if not d.eof and len(raw) <= expect:
                raise zlib.error('incomplete or truncated stream')
        except zlib.error as e:
            raise ValueError(f'{where}: {e}') from None
    if len(raw) != expect:
        raise ValueError(f'{where}: {len(raw)} bytes, defaultArrayLength promises {expect}')
    return raw


def _array(spectrum, accession, n, where):
    for bda in _descendants(spectrum, 'binaryDataArray'):
        kinds = _params(bda, ('MS:1000514', 'MS:1000515'))
        if not kinds or kinds[0].get('accession') != accession:
            continue
        binary = _children(bda, 'binary')
        if not binary:
            break
        prec = _params(bda, set(_PRECISION) | _BAD_PRECISION)
        comp = _params(bda, set(_COMPRESSION) | _BAD_COMPRESSION)
        if not prec or prec[0].get('accession') not in _PRECISION:
            raise ValueError(f'{where}: a missing or unsupported precision')
        if not comp or comp[0].get('accession') not in _COMPRESSION:
            raise ValueError(f'{where}: a missing or unsupported compression')
        dtype = _PRECISION[prec[0].get('accession')]
        raw = decode((binary[0].text or '').encode('ascii', 'replace'), _COMPRESSION[comp[0].get('accession')],
                     n * int(dtype[2]), where)
        return np.frombuffer(raw, dtype)
    raise ValueError(f'{where}: no {"m/z" if accession == "MS:1000514" else "intensity"} array')


def scan_identifier(spectrum_id: str):
    for key in ('scan=', 'index='):
        if key in spectrum_id:
            try:
                return str(int(spectrum_id[spectrum_id.find(key) + len(key):]))
            except ValueError:
                return None
    return None


def read_mzml(source):
    if isinstance(source, (str, os.PathLike)):
        with open(source, 'rb') as f:
            data = f.read()
    else:
        data = bytes(source)
    first = _SPECTRUM.search(data)
    if first is not None:
        marks = [p for p in (data.find(b'<!--', first.start()), data.find(b'<![CDATA[', first.start())) if p >= 0]
        if marks:
            k = len(_SPECTRUM.findall(data, 0, min(marks)))
            raise ValueError(f'spectrum {k - 1}: a comment or CDATA section after the first <spectrum')
    root = ET.fromstring(data)
    out = []
    for index, sp in enumerate(e for e in root.iter() if _local(e) == 'spectrum'):
        level = _params(sp, ('MS:1000511',))
        value = level[0].get('value') if level else None
        if value is None or not _DIGITS.fullmatch(value) or int(value) != 2:
            continue
        where = f'spectrum {index}'
        # what fails while pyteomics iterates over the file
        if _descendants(sp, 'referenceableParamGroupRef'):
            raise ValueError(f'{where}: a referenceableParamGroupRef')
        if any(b.get('arrayLength') is not None for b in _descendants(sp, 'binaryDataArray')):
            raise ValueError(f'{where}: an arrayLength attribute')
        n = sp.get('defaultArrayLength')
        if n is None or not _DIGITS.fullmatch(n):
            raise ValueError(f'{where}: defaultArrayLength {n!r}')
        n = int(n)
        if n > MAX_PEAKS:
            raise OverflowError(f'{where}: more than {MAX_PEAKS} peaks')
        mz = _array(sp, 'MS:1000514', n, where)
        intensity = _array(sp, 'MS:1000515', n, where)
        if sp.get('id') is None:
            raise ValueError(f'{where}: no id')
        # the reference's parser: the identifier first
        identifier = scan_identifier(sp.get('id'))
        if identifier is None:
            logging.warning('mzML: failed to read spectrum %s: no scan or index number in its id', sp.get('id'))
            continue
        scans = [s for sl in _children(sp, 'scanList') for s in _children(sl, 'scan')]
        rt = _params(scans[0], ('MS:1000016',)) if scans else []
        if not rt:
            raise ValueError(f'{where}: no scan start time')
        rt = _number(rt[0].get('value'), where, 'scan start time')
        precursors = [p for pl in _children(sp, 'precursorList') for p in _children(pl, 'precursor')]
        ions = _descendants(precursors[0], 'selectedIon') if precursors else []
        pmz = _params(ions[0], ('MS:1000744',)) if ions else []
        if not pmz:
            raise ValueError(f'{where}: no precursor with a selected ion m/z')
        pmz = _number(pmz[0].get('value'), where, 'selected ion m/z')
        state, possible = _params(ions[0], ('MS:1000041',)), _params(ions[0], ('MS:1000633',))
        if state:
            z = _charge(state[0].get('value'), where)
        elif len(possible) == 1:
            z = _charge(possible[0].get('value'), where)
        elif possible:
            raise ValueError(f'{where}: several possible charge states')
        else:
            z = None
        out.append(SimpleNamespace(identifier=identifier, precursor_mz=pmz, precursor_charge=z, mz=mz,
                                   intensity=intensity, retention_time=rt, index=index))
    return out
