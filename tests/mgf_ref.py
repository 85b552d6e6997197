"""The MGF dialect of ``ann_solo_amd.mgf`` restated in plain Python: the definition the device reader is
tested against (include/annsolo_mi.h "MGF query files", DESIGN.md 3 "Query files").

The rules are what the reference's ``read_mgf`` (reader.py:868-911) reads through pyteomics' ``mgf.MGF`` with
``use_header=True``, written down from its documented behaviour. pyteomics is not a dependency of this
project, so the restatement is unpinned and IS the definition. The deviations -- cases where the reference
crashes or yields garbage -- raise ``ValueError`` naming the 1-based line or spectrum.

``read_mgf(source)`` takes a path or bytes and returns the list of spectrum objects ``pack_queries`` takes.
"""
import logging
import math
import os
import re
from types import SimpleNamespace

import numpy as np

_CHARGE_SPLIT = re.compile(rb'(?:,\s*)|(?:\s*and\s*)')
_CHARGE = re.compile(rb'([+-]?)([0-9]+)|([0-9]+)([+-])')


def parse_charge(value: bytes, where: str) -> int:
    """The first element of pyteomics' charge list: 1 .. 255."""
    first = _CHARGE_SPLIT.split(value)[0].strip()
    m = _CHARGE.fullmatch(first)
    if m is None:
        raise ValueError(f'{where}: charge {value!r} is not a charge')
    sign = m.group(1) if m.group(2) is not None else m.group(4)
    digits = m.group(2) if m.group(2) is not None else m.group(3)
    z = -int(digits) if sign == b'-' else int(digits)
    if not 1 <= z <= 255:
        raise ValueError(f'{where}: charge {z} outside 1 .. 255')
    return z


def _number(token: bytes, where: str, what: str) -> float:
    try:
        v = float(token)
    except ValueError:
        raise ValueError(f'{where}: {what} {token!r} is not a number') from None
    if not math.isfinite(v):
        raise ValueError(f'{where}: non-finite {what} {token!r}')
    return v


def read_mgf(source):
    if isinstance(source, (str, os.PathLike)):
        with open(source, 'rb') as f:
            data = f.read()
    else:
        data = bytes(source)
    lines = data.split(b'\n')
    if lines and lines[-1] == b'':
        lines.pop()
    header, params, mzs, its = {}, None, None, None
    seen_block = False
    out = []
    for no, raw in enumerate(lines, 1):
        line = raw.strip()
        if params is None:                       # outside a block
            if line == b'BEGIN IONS':
                params, mzs, its, seen_block = dict(header), [], [], True
            elif not seen_block and b'=' in line and line[:1] not in (b'#', b';', b'!', b'/'):
                k, v = line.split(b'=', 1)
                header[k.lower()] = v.strip()
            continue
        if not line or line[:1] in (b'#', b';', b'!', b'/'):
            continue
        if line == b'END IONS':
            index = len(out) + 1
            where = f'spectrum {index}'
            ident = params.get(b'title', params.get(b'scan'))
            if ident is None:
                raise ValueError(f'{where}: neither TITLE nor SCAN')
            if b'pepmass' not in params:
                raise ValueError(f'{where}: no PEPMASS')
            tok = params[b'pepmass'].split()
            pmz = _number(tok[0] if tok else b'', where, 'pepmass')
            z = parse_charge(params[b'charge'], where) if b'charge' in params else None
            rt = _number(params[b'rtinseconds'], where, 'rtinseconds') if b'rtinseconds' in params else None
            out.append(SimpleNamespace(identifier=ident.decode('utf-8'), precursor_mz=pmz, precursor_charge=z,
                                       mz=np.asarray(mzs, np.float64), intensity=np.asarray(its, np.float64),
                                       retention_time=rt, index=index))
            params = None
            continue
        if line == b'BEGIN IONS':
            raise ValueError(f'line {no}: BEGIN IONS inside a block')
        if b'=' in line:
            k, v = line.split(b'=', 1)
            params[k.lower()] = v.strip()        # the last duplicate wins
            continue
        tok = line.split()
        if len(tok) < 2:
            raise ValueError(f'line {no}: a peak line with one token')
        mzs.append(_number(tok[0], f'line {no}', 'm/z'))
        its.append(_number(tok[1], f'line {no}', 'intensity'))
    if params is not None:
        logging.warning('MGF: the last block is not closed at the end of the file: dropped')
    return out
