"""Cases for the .sptxt reader: annotation strings for the fragment-charge rule, and the builders of the small
SpectraST text files the tests read (``tests/sptxt_ref.py`` is what they are read against)."""
import numpy as np

RESIDUES = 'ACDEFGHIKLMNPQRSTVWY'
MOD_NAMES = ('Carbamidomethyl', 'Oxidation', 'Acetyl', 'Phospho', 'Deamidated')
TAILS = ['5', '5-18', '5^2', '5-17^3/0.01', '^', '^x', '', '5/0.1,b3^2/0.2']
ANNOTATIONS = ['b5/0.01', 'y7^2/0.02', 'y3-18^2/0.01,b4/0.3', '?', 'p^3/0.0', 'a2', 'IKD/0.0', '', 'y11^3i/0.1',
               'b2-17/0.05', 'p-18^2/0.0', '? 3/4']


def annotation_cases():
    """Every first character of printable ASCII with each tail, and a few more."""
    out = [chr(c) + t for c in range(32, 127) for t in TAILS]
    return out + ['', 'y', 'y^', 'y^0', 'y^12', 'y^255', 'y^256', 'y^99999999999', 'b3/0.1^2', 'b3^2^3', 'y^ 2',
                  'Y5^2', 'b5^2i', ' b5^2', 'p^2/0.0,y3^3']


def random_annotations(n: int, seed: int):
    rng = np.random.default_rng(seed)
    alphabet = 'abyp?IKx^^^//0123456789-,. i'
    heads = ['', 'a', 'b', 'y', 'p', 'y1', 'b12', 'y3^', 'b7-18^', 'p^']      # most of them annotated
    return [heads[int(rng.integers(0, len(heads)))] +
            ''.join(alphabet[int(k)] for k in rng.integers(0, len(alphabet), int(rng.integers(0, 12))))
            for _ in range(n)]


# ---------------------------------------------------------------------------------------------- files
def peptide(rng, length=None) -> str:
    length = int(rng.integers(7, 16)) if length is None else length
    return ''.join(RESIDUES[int(k)] for k in rng.integers(0, len(RESIDUES), length - 1)) + 'KR'[int(rng.integers(0, 2))]


def mods_value(rng, pep: str, n_mods=None) -> str:
    n_mods = int(rng.integers(0, 3)) if n_mods is None else n_mods
    idx = np.sort(rng.integers(0, len(pep), n_mods))
    return '/'.join([str(n_mods)] + ['%d,%s,%s' % (i, pep[int(i)], MOD_NAMES[int(rng.integers(0, len(MOD_NAMES)))])
                                     for i in idx])


def peak_lines(rng, n_peaks, order='ascending', annotated=True):
    mz = np.sort(rng.uniform(100.0, 1500.0, n_peaks))
    if order == 'descending':
        mz = mz[::-1]
    elif order == 'shuffled':
        mz = rng.permutation(mz)
    it = rng.uniform(1.0, 10000.0, n_peaks)
    ann = [ANNOTATIONS[int(rng.integers(0, len(ANNOTATIONS)))] if annotated else '?' for _ in range(n_peaks)]
    return ['%.4f\t%.1f\t%s\t%d/%d 0.%d' % (a, b, c, rng.integers(1, 9), 9, rng.integers(1, 9))
            for a, b, c in zip(mz, it, ann)]


def record(rng, charge=2, n_peaks=None, pep=None, precursor='both', decoy=None, newline='\n', order='ascending',
           comment_extra='', peaks=None, numpeaks='NumPeaks: %d', mods=True):
    """One record in the shape SpectraST writes; ``precursor``: 'both', 'line' (PrecursorMZ only), 'parent'."""
    n_peaks = int(rng.integers(12, 41)) if n_peaks is None else n_peaks
    pep = peptide(rng) if pep is None else pep
    pmz = rng.uniform(300.0, 1200.0)
    name = 'Name: %s%s/%d' % ('DeCoY_1 ' if decoy == 'name' else '', pep, charge)
    comment = 'Comment: AvePrecursorMz=%.4f BinaryFileOffset=%d Fullname=K.%s.L/%d' % (pmz + 0.3, rng.integers(1, 10**9),
                                                                                       pep, charge)
    if mods:
        comment += ' Mods=' + mods_value(rng, pep)
    if precursor in ('both', 'parent'):
        comment += ' Parent=%.3f' % (pmz if precursor == 'parent' else pmz + 1.0)
    comment += ' Protein=1/sp|P%05d|%s Spec=Consensus%s' % (rng.integers(0, 99999),
                                                            'DECOY_X' if decoy == 'comment' else 'TARGET_X', comment_extra)
    lines = [name, 'LibID: %d' % rng.integers(0, 10**6), 'MW: %.4f' % (pmz * charge)]
    if precursor in ('both', 'line'):
        lines.append('PrecursorMZ: %.4f' % pmz)
    lines += ['Status: Normal', 'FullName: K.%s.L/%d (CID)' % (pep, charge), comment]
    peaks = peak_lines(rng, n_peaks, order) if peaks is None else peaks
    lines.append(numpeaks % len(peaks))
    return newline.join(lines + list(peaks) + ['']) + newline


PREAMBLE = '### a consensus library written by hand\n### FullName: not a record; rename: neither\n###\n'


def plain_file(n_records: int, seed: int, newline='\n', preamble=False, charges=(2, 3, 2, 1, 3, 2), **kw) -> bytes:
    """Charges 1 to 4 mixed; charge 4 occurs once where the file has more than two records."""
    rng = np.random.default_rng(seed)
    out = [PREAMBLE.replace('\n', newline)] if preamble else []
    for i in range(n_records):
        z = 4 if (i == 2 and n_records > 2) else charges[i % len(charges)]
        out.append(record(rng, charge=z, newline=newline, precursor=('both', 'line', 'parent')[i % 3], **kw))
    return ''.join(out).encode('utf-8')


# ---------------------------------------------------------------------------------------------- refusals
def small_record(name='Name: ACDEK/2', meta=('PrecursorMZ: 500.25', 'Comment: Mods=0 Spec=x'), numpeaks='NumPeaks: 2',
                 peaks=('100.5\t1\tb1', '200.5\t2\ty1^2')) -> str:
    """Six lines as it stands: Name, two metadata lines, Num Peaks, two peaks."""
    return '\n'.join([name, *meta] + ([numpeaks] if numpeaks is not None else []) + list(peaks)) + '\n'


def _refusals():
    good = small_record()
    pmz = 'PrecursorMZ: 500.25'
    out = []
    add = lambda where, before='', after='', **kw: out.append(((before + good + small_record(**kw) + after).encode(),
                                                               where))
    # lines: 7 Name, 8 and 9 metadata, 10 Num Peaks, 11 and 12 peaks (one more with a preamble line)
    add('line 9', meta=(pmz, 'Comment: see Name: other'))
    add('line 7', name='Name: AAK/2 Name: CCK/2', after=good)
    add('line 11', peaks=('100.5\t1\tb1 name: x', '200.5\t2\ty1'))
    add('line 1', before='### see Name: x\n')
    add('line 12', peaks=('100.5\t1\tb1', 'Num Peaks: 3', '200.5\t2\ty1'))
    for bad in ('NumPeaks: x', 'NumPeaks: 2 3', 'NumPeaks:  2', 'NumPeaks:', 'NumPeaks: 2_0'):
        add('line 10', numpeaks=bad)
    for bad in ('100.5\t1', '100.5 1 b1', '100.5'):
        add('line 11', peaks=(bad, '200.5\t2\ty1'), after=good)
    for bad in ('PrecursorMZ: 500.25 x', 'PrecursorMZ: .5', 'PrecursorMZ: 1e3', 'PrecursorMZ:  500.25', 'PrecursorMZ:',
                'PrecursorMZ: 5.', 'PrecursorMZ: 1.2.3', 'PrecursorMZ: 5_0.5'):
        add('line 8', meta=(bad, 'Comment: x'))
    for bad in ('Comment: x PrecursorMZ: 5.5', 'Comment: NumPeaks: 3', 'Comment: AvePrecursorMZ: 5.5 x',
                'Comment: Spec=a Num Peaks: 2'):
        add('line 9', meta=(pmz, bad))                                # keys the reference finds inside a line
    add('line 7', name='Name: AAK/2 NumPeaks: 2', after=good)
    add('line 9', meta=(pmz, 'PrecursorMZ: x'))                       # a later PrecursorMZ line is checked too
    for bad in ('Name: AAAK/2_0', 'Name: AAAK/0', 'Name: AAAK/256', 'Name: AAAK', 'Name: AAAK/+2', 'Name: AAAK/',
                'Name: AAAK/2 x', 'Name: n[43]AAAK/2', 'Name: aaak/2', 'Name: A[Oxidation]AK/2', 'Name:AAAK/2',
                'Name: /2'):
        add('record 2', name=bad, after=good)
        add('record 2', name=bad)
    for bad in ('Comment: x', 'Comment: Parent=.5 x', 'Comment: Parent=5. x', 'Comment: Parent=abc', 'Comment: Parent=',
                'Comment: Parent=  5.5', 'Comment: Parent=.5 Parent=5.5', 'Comment: Mods=1/9,K,Phospho Parent=5.5',
                'Comment: Parent=5.5 Mods=1/1,C', 'Comment: Mods=1/-2,A,Acetyl Parent=5.5',
                'Comment: Parent=5.5 Mods=2/3,E,X/1,C,Y'):
        add('record 2', meta=(bad,), after=good)
    add('record 2', peaks=())
    add('record 2', peaks=(), after=good)
    add('record 2', peaks=('# only a comment', '   ', ''), after=good)
    add('record 2', numpeaks=None, peaks=())
    add('record 2', numpeaks='Num  Peaks: 2')                         # no key: the peaks are metadata
    for bad in ('abc\t1\tb1', '100.5\tnan\tb1', '100.5\t1e999\tb1', '\t1\tb1', '1 0\t1\tb1', '100.5\t\tb1', 'inf\t1\tb1'):
        add('line 11', peaks=(bad, '200.5\t2\ty1'), after=good)
    # the first of two: a record-level error stands behind its record, before a later line's
    out.append(((good + small_record(name='Name: AAAK/0') + small_record(peaks=('x\t1\tb1',))).encode(), 'record 2'))
    out.append(((good + small_record(peaks=('x\t1\tb1',)) + small_record(name='Name: AAAK/0')).encode(), 'line 11'))
    return out


REFUSALS = _refusals()
