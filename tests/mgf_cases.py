"""Cases for the MGF reader: the numeral rule stated a second time (``needs_host``: a regular expression and
Python integers, no floating point), the edge numerals of the issue, seeded random numerals, and the builders
of the small MGF files the GPU tests read."""
import re

import numpy as np

_NUMERAL = re.compile(rb'[+-]?(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?')


def needs_host(token: bytes) -> bool:
    """True where the device must NOT convert ``token`` itself (include/annsolo_mi.h, asl_mgf_number)."""
    m = _NUMERAL.fullmatch(token)
    if m is None:
        return True
    whole, frac = (m.group(1), m.group(2) or b'') if m.group(1) is not None else (b'', m.group(3))
    digits = (whole + frac).lstrip(b'0')
    if not digits:
        return False                        # a zero converts at any exponent
    if len(digits) > 19 or int(digits) >= 1 << 53:
        return True
    e = int(m.group(4) or 0) - len(frac)
    return not -22 <= e <= 22


EDGES = [
    str(2 ** 53 - 1), str(2 ** 53), str(2 ** 53 - 1) + '.0', str(2 ** 53) + 'e-3',
    '9' * 15, '9' * 16, '9' * 17, '0.' + '9' * 15, '0.' + '9' * 16, '9.' + '9' * 16,
    '1e22', '1e23', '1e-22', '1e-23', '123456789012345e22', '1.5e23', '15e-23', '1.5e-22',
    '-0', '-0.0e400', '0e-999', '+0.000',
    '.5', '5.', '+1', '007.50', '-.25e1', '5.e2', '1E5', '1e+5',
    '0' * 400 + '1.5', '0.' + '0' * 400 + '1', '0' * 400,
    '1234567890123456789', '12345678901234567890', '0.1234567890123456789', '1000000000000000000000',
    '1e400', '-1e400', '1e-400', 'nan', 'inf', '-inf', 'Infinity', '1_0', '1e', 'e5', '.', '+', '', '1.2.3',
    '0x10', '1,5', '12abc', '--1', '1e5.0', '\xb5', '4.9e-324', '1.7976931348623157e308', '2.2250738585072014e-308',
]
EDGES = [e.encode('utf-8') if e != '\xb5' else b'\xb5' for e in EDGES]
# of the edges, what Python's float() itself refuses (a ValueError in a file)
REFUSED = [b'1e', b'e5', b'.', b'+', b'', b'1.2.3', b'0x10', b'1,5', b'12abc', b'--1', b'1e5.0', b'\xb5']
NON_FINITE = [b'1e400', b'-1e400', b'nan', b'inf', b'-inf', b'Infinity']


def random_numerals(n: int, seed: int):
    """Numerals of 1 to 17 digits, with and without point, exponent and sign."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        nd = int(rng.integers(1, 18))
        digits = ''.join(str(d) for d in rng.integers(0, 10, nd))
        point = int(rng.integers(0, nd + 2))            # nd + 1: no point
        s = digits if point > nd else digits[:point] + '.' + digits[point:]
        if s == '.':
            s = '0.'
        if rng.random() < 0.4:
            s += 'eE'[int(rng.integers(0, 2))] + ['', '+', '-'][int(rng.integers(0, 3))] + str(int(rng.integers(0, 31)))
        s = ['', '+', '-'][int(rng.integers(0, 3))] + s
        out.append(s.encode('ascii'))
    return out


# ---------------------------------------------------------------------------------------------- files
def spectrum_block(rng, title, n_peaks=None, charge='2+', rt=True, descending=False, newline='\n', extra=()):
    """One block whose spectrum survives the default preprocessing (>= 10 peaks over >= 250 m/z)."""
    n_peaks = int(rng.integers(12, 40)) if n_peaks is None else n_peaks
    mz = np.sort(rng.uniform(100.0, 1500.0, n_peaks))
    if descending:
        mz = mz[::-1]
    it = rng.uniform(1.0, 1000.0, n_peaks)
    lines = ['BEGIN IONS', f'TITLE={title}', 'PEPMASS=%.5f %.1f' % (rng.uniform(300.0, 1200.0), rng.uniform(1, 9))]
    if charge is not None:
        lines.append(f'CHARGE={charge}')
    if rt:
        lines.append('RTINSECONDS=%.3f' % rng.uniform(0.0, 7200.0))
    lines.extend(extra)
    lines.extend('%.4f %.2f' % (a, b) for a, b in zip(mz, it))
    lines.append('END IONS')
    return newline.join(lines) + newline


def plain_file(n_spectra: int, seed: int, newline='\n', charges=('2+', '3+', None, '2')) -> bytes:
    rng = np.random.default_rng(seed)
    return ''.join(spectrum_block(rng, f'spec {i} scan={i}', charge=charges[i % len(charges)], newline=newline)
                   for i in range(n_spectra)).encode('utf-8')


def file_of_lines(n_lines: int, seed: int) -> bytes:
    """A file of exactly ``n_lines`` lines: whole blocks, the last one sized to fit."""
    rng = np.random.default_rng(seed)
    out, left, i = [], n_lines, 0
    while left > 0:
        fixed = 6                            # BEGIN, TITLE, PEPMASS, CHARGE, RT, END
        n_peaks = 20 if left >= 2 * (fixed + 20) else left - fixed
        if n_peaks < 12:                     # (cannot happen for the line counts the tests use)
            raise ValueError(n_lines)
        out.append(spectrum_block(rng, f't{i}', n_peaks=n_peaks))
        left -= fixed + n_peaks
        i += 1
    data = ''.join(out).encode('utf-8')
    assert data.count(b'\n') == n_lines
    return data


HAND_WRITTEN = b'''# a hand-written file: about thirty lines\r
CHARGE=2+ and 3+\r
INSTRUMENT=Default
; a comment in the header
some text before the first block
BEGIN IONS
TITLE=first = one
PEPMASS=500.25 1234.5
RTINSECONDS=12.5
100.5 10
   200.25\t20   2+

! a comment inside
300.125 30 and more
END IONS
between the blocks
END IONS
BEGIN IONS\r
SCAN=17\r
PEPMASS=400.5\r
PEPMASS=600.75\r
CHARGE=3+\r
charge=4\r
150.5 1.5\r
50.25 2.5\r
END IONS\r
BEGIN IONS
TITLE=
SCAN=9
PEPMASS=.5e3
CHARGE=
CHARGE=1,2
7 8
END IONS
BEGIN IONS
TITLE=never closed
PEPMASS=1
1 2'''
