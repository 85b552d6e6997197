"""The .sptxt dialect of ``ann_solo_amd.sptxt`` restated in plain Python: the definition the device reader is
tested against (include/annsolo_mi.h "Library files", DESIGN.md 3 "Library files").

The rules are the well-formed subset of what the reference's SpectraST text reader accepts, written down from
its documented behaviour with ``re`` and numpy only. pyteomics and spectrum_utils are not dependencies of this
project, so the restatement is unpinned and IS the definition. Everything outside the subset raises ``ValueError``
naming the 1-based line or record.

``read_sptxt(source)`` takes a path or bytes and returns the list of spectrum objects ``pack_raw`` takes.
"""
import math
import os
import re
from types import SimpleNamespace

import numpy as np

_SECOND_NAME = re.compile(rb'(?<![a-z])name:')
_NUMPEAKS_KEY = re.compile(rb'num\s?peaks:')
_NUMPEAKS_LINE = re.compile(rb'num\s?peaks:\s?[0-9]+')
_PRECURSOR_LINE = re.compile(rb'precursormz:\s?([0-9]+(?:\.[0-9]+)?)')
_RUN = re.compile(rb'\s?([0-9.]*)')
_NUMERAL = re.compile(rb'[0-9]+(?:\.[0-9]+)?')
_CHARGE = re.compile(rb'[0-9]+')
_LEADING_DIGITS = re.compile(r'[0-9]+')


def fragment_charge(annotation: str) -> int:
    """0 for an unannotated peak: an empty field or a first character other than a, b, y, p. Else the number
    behind the ``^`` of the first annotation (the text before the first ``/``), capped at 255; 1 without one."""
    if annotation[:1] not in ('a', 'b', 'y', 'p'):
        return 0
    pieces = annotation[1:].split('/', 1)[0].split('^')
    if len(pieces) == 1:
        return 1
    m = _LEADING_DIGITS.match(pieces[1])
    return min(int(m.group(0)), 255) if m else 1


def proforma(peptide: str, mods) -> str:
    """Residue by residue: the letter, then ``[name]`` for every modification listed at its index; those listed at
    -1 come first of all. ``mods``: the value of ``Mods=`` (``count/index,residue,name/...``) or None."""
    if not peptide or any(not ('A' <= a <= 'Z') for a in peptide):
        raise ValueError(f'peptide {peptide!r} is not upper-case letters only')
    at = {i: [] for i in range(-1, len(peptide))}
    last = -1
    for field in ([] if mods is None else mods.split('/')[1:]):
        parts = field.split(',')
        if len(parts) != 3 or re.fullmatch(r'-?[0-9]+', parts[0]) is None:
            raise ValueError(f'modification {field!r} is not index,residue,name')
        i = int(parts[0])
        if i not in at or i < last:
            raise ValueError(f'modification {field!r}: index outside -1 .. {len(peptide) - 1}, or descending')
        last = i
        at[i].append('[' + parts[2] + ']')
    return ''.join(at[-1]) + ''.join(a + ''.join(at[i]) for i, a in enumerate(peptide))


def _number(token: bytes, where: str, what: str) -> float:
    try:
        v = float(token)
    except ValueError:
        raise ValueError(f'{where}: {what} {token!r} is not a number') from None
    if not math.isfinite(v):
        raise ValueError(f'{where}: non-finite {what} {token!r}')
    return v


class _Record:
    def __init__(self, ordinal, name_line):
        self.ordinal, self.name_line = ordinal, name_line
        self.precursor_line = self.parent = self.mods = None
        self.decoy = False
        self.mz, self.intensity, self.charge = [], [], []

    def metadata(self, line: bytes, low: bytes) -> None:
        """A metadata line that is no PrecursorMZ line (the Name line is one of them)."""
        self.decoy = self.decoy or b'decoy' in low
        if self.parent is None and b'parent=' in low:
            run = _RUN.match(low, low.index(b'parent=') + 7).group(1)
            self.parent = run if _NUMERAL.fullmatch(run) else False
        if self.mods is None and b'mods=' in low:
            self.mods = re.match(rb'\S*', line[low.index(b'mods=') + 5:]).group(0)

    def close(self):
        where = f'record {self.ordinal}'
        head = self.name_line.split(b'/')
        if len(head) < 2:
            raise ValueError(f'{where}: the Name line has no "/"')
        charge = head[1].strip()
        if _CHARGE.fullmatch(charge) is None or not 1 <= int(charge) <= 255:
            raise ValueError(f'{where}: precursor charge is not digits in 1 .. 255')
        try:
            peptide = proforma(head[0].split(b' ')[-1].strip().decode('utf-8', 'replace'),
                               None if self.mods is None else self.mods.decode('utf-8', 'replace'))
        except ValueError as e:
            raise ValueError(f'{where}: {e}') from None
        token = self.precursor_line if self.precursor_line is not None else self.parent
        if token is None:
            raise ValueError(f'{where}: neither a PrecursorMZ line nor Parent=')
        if token is False:
            raise ValueError(f'{where}: the Parent= numeral is not digits[.digits]')
        if not self.mz:
            raise ValueError(f'{where}: no peak lines')
        return SimpleNamespace(identifier=str(self.ordinal), precursor_mz=_number(token, where, 'precursor m/z'),
                               precursor_charge=int(charge), mz=np.asarray(self.mz, np.float64),
                               intensity=np.asarray(self.intensity, np.float64),
                               annotation=[SimpleNamespace(charge=z) if z else None for z in self.charge],
                               peptide=peptide, is_decoy=self.decoy, retention_time=None)


def read_sptxt(source):
    if isinstance(source, (str, os.PathLike)):
        with open(source, 'rb') as f:
            data = f.read()
    else:
        data = bytes(source)
    lines = data.split(b'\n')
    if lines and lines[-1] == b'':
        lines.pop()
    out, rec, in_peaks = [], None, False
    for no, raw in enumerate(lines, 1):
        line = raw.strip()
        low = line.lower()
        if any(m.start() > 0 for m in _SECOND_NAME.finditer(low)):
            raise ValueError(f'line {no}: a second Name: in the line')
        is_name = low.startswith(b'name:')
        is_key = _NUMPEAKS_KEY.match(low) is not None or low.startswith(b'precursormz:')
        if (is_name or (rec is not None and not in_peaks and not is_key)) and \
                (_NUMPEAKS_KEY.search(low, 1) or low.find(b'precursormz:', 1) >= 0):
            raise ValueError(f'line {no}: a PrecursorMZ: or Num Peaks: key inside a metadata line')
        if is_name:
            if rec is not None:
                out.append(rec.close())
            rec, in_peaks = _Record(len(out) + 1, line), False
            rec.metadata(line, low)
        elif rec is None:
            continue                                 # the preamble
        elif _NUMPEAKS_KEY.match(low):
            if in_peaks:
                raise ValueError(f'line {no}: a second Num Peaks line in the record')
            if _NUMPEAKS_LINE.fullmatch(low) is None:
                raise ValueError(f'line {no}: a Num Peaks line that is not "Num Peaks: <digits>"')
            in_peaks = True
        elif not in_peaks:
            if low.startswith(b'precursormz:'):
                m = _PRECURSOR_LINE.fullmatch(low)
                if m is None:
                    raise ValueError(f'line {no}: a PrecursorMZ line that is not "PrecursorMZ: <digits[.digits]>"')
                if rec.precursor_line is None:
                    rec.precursor_line = m.group(1)
            else:
                rec.metadata(line, low)
        else:
            cut = raw.split(b'#', 1)[0] if b'#' in raw else raw.rstrip(b'\r\n')
            if not cut.strip():
                continue
            fields = cut.split(b'\t')
            if len(fields) < 3:
                raise ValueError(f'line {no}: a peak line with fewer than three fields')
            rec.mz.append(_number(fields[0].strip(), f'line {no}', 'm/z'))
            rec.intensity.append(_number(fields[1].strip(), f'line {no}', 'intensity'))
            rec.charge.append(fragment_charge(fields[2].decode('latin-1')))
    if rec is not None:
        out.append(rec.close())
    return out
