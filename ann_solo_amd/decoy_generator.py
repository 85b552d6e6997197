"""Shuffle-and-reposition decoys (the reference's ``decoy_generator.shuffle_and_reposition``,
/root/reference/src/ann_solo/decoy_generator.py:10-185) for whole batches of library spectra.

The shuffle (``shuffle``: tryptic residues stay, up to 10 draws, the first at most 70 % similar wins)
and the peptide parser run on the host; the annotation of every peak with the peptide's a / b / p / y
fragments, the repositioning onto the shuffled peptide's fragments and the re-sort are one HIP kernel
(``asl_decoy_batch``, csrc/decoy.hip; the arithmetic is written down in include/annsolo_mi.h and
DESIGN.md 3 "Decoys"). The random stream is this module's own: one ``PCG64`` generator per peptide,
seeded from (seed, peptide string, precursor charge), so a spectrum's decoy depends neither on its
batch nor on its row.
"""
import ctypes as C
import hashlib
import re
from dataclasses import dataclass
from difflib import ndiff
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

RESIDUE_MASS = {
    'G': 57.021464, 'A': 71.037114, 'S': 87.032028, 'P': 97.052764, 'V': 99.068414, 'T': 101.047679,
    'C': 103.009185, 'L': 113.084064, 'I': 113.084064, 'N': 114.042927, 'D': 115.026943,
    'Q': 128.058578, 'K': 128.094963, 'E': 129.042593, 'M': 131.040485, 'H': 137.058912,
    'F': 147.068414, 'R': 156.101111, 'Y': 163.063329, 'W': 186.079313}
MODIFICATION_MASS = {'Carbamidomethyl': 57.021464, 'Oxidation': 15.994915, 'Acetyl': 42.010565,
                     'Phospho': 79.966331, 'Deamidated': 0.984016}
EXCLUDED_RESIDUES = ('K', 'R', 'P')
MAX_SIMILARITY = 0.7
N_DRAWS = 10
BATCH = 32768
_NUMBER = re.compile(r'^[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?$')


@dataclass
class Peptide:
    """A parsed peptide: residue letters, the mass difference on every residue (0.0: unmodified) and
    the terminal additions, which the shuffle leaves where they are."""
    sequence: str
    deltas: Tuple[float, ...]
    nterm: float = 0.0
    cterm: float = 0.0

    @property
    def masses(self) -> np.ndarray:
        """Residue masses with the modifications folded in (one fp64 add each)."""
        return np.asarray([RESIDUE_MASS[a] + d for a, d in zip(self.sequence, self.deltas)], np.float64)

    def permuted(self, perm: Sequence[int]) -> 'Peptide':
        return Peptide(''.join(self.sequence[i] for i in perm), tuple(self.deltas[i] for i in perm),
                       self.nterm, self.cterm)

    def __str__(self) -> str:
        tag = lambda d: '[%s]' % (('%+.6f' % d).rstrip('0').rstrip('.'))
        body = ''.join(a + (tag(d) if d else '') for a, d in zip(self.sequence, self.deltas))
        return (tag(self.nterm) + '-' if self.nterm else '') + body + ('-' + tag(self.cterm) if self.cterm else '')


def _tag_mass(tag: str, table: Dict[str, float], peptide: str, where) -> float:
    if _NUMBER.match(tag):
        return float(tag)
    if tag in table:
        return float(table[tag])
    raise ValueError(f'unknown modification [{tag}] in peptide {peptide!r}'
                     + (f' of spectrum {where!r}' if where is not None else ''))


def parse_peptide(peptide: str, modification_masses: Optional[Dict[str, float]] = None,
                  spectrum=None) -> Peptide:
    """``X[+m]`` / ``X[m]`` (a mass difference in Da) or ``X[Name]`` (``MODIFICATION_MASS``, extended or
    overridden by ``modification_masses``) on any residue; ``[tag]-`` in front and ``-[tag]`` behind are
    the terminal additions. An unknown name or residue letter is a
    ``ValueError`` that names it and ``spectrum`` (an identifier for the message): no mass is guessed."""
    table = dict(MODIFICATION_MASS)
    if modification_masses:
        table.update(modification_masses)
    if not isinstance(peptide, str) or not peptide:
        raise ValueError(f'no peptide for spectrum {spectrum!r}: decoys need the sequence')
    text = peptide.strip()
    nterm = cterm = 0.0
    m = re.match(r'^\[([^\]]*)\]-', text)
    if m:
        nterm, text = _tag_mass(m.group(1), table, peptide, spectrum), text[m.end():]
    m = re.search(r'-\[([^\]]*)\]$', text)
    if m:
        cterm, text = _tag_mass(m.group(1), table, peptide, spectrum), text[:m.start()]
    seq, deltas, i = [], [], 0
    while i < len(text):
        a = text[i]
        if a not in RESIDUE_MASS:
            raise ValueError(f'unknown residue {a!r} in peptide {peptide!r}'
                             + (f' of spectrum {spectrum!r}' if spectrum is not None else ''))
        i += 1
        d = 0.0
        while i < len(text) and text[i] == '[':
            j = text.find(']', i)
            if j < 0:
                raise ValueError(f'unclosed modification tag in peptide {peptide!r}')
            d += _tag_mass(text[i + 1:j], table, peptide, spectrum)
            i = j + 1
        seq.append(a)
        deltas.append(d)
    return Peptide(''.join(seq), tuple(deltas), nterm, cterm)


def peptide_rng(seed: int, peptide: str, charge: int) -> np.random.Generator:
    h = hashlib.sha256(f'{int(seed)}|{peptide}|{int(charge)}'.encode('utf-8')).digest()
    return np.random.Generator(np.random.PCG64(int.from_bytes(h[:16], 'little')))


def shuffle(sequence: str, rng: np.random.Generator) -> Tuple[str, List[int]]:
    """``(shuffled, perm)`` with ``shuffled[i] == sequence[perm[i]]``. K, R and P among the first L - 1
    residues and the last residue keep their places; of up to 10 draws the first whose similarity to
    ``sequence`` (1 - differing ``ndiff`` lines / L) is at most 0.7 wins, else the least similar one.
    Nothing to permute: the sequence itself."""
    seq = list(sequence)
    L = len(seq)
    movable = [i for i in range(L - 1) if seq[i] not in EXCLUDED_RESIDUES]
    best_similarity, best = 1.0, list(range(L))
    if len(movable) < 2:
        return sequence, best
    for _ in range(N_DRAWS):
        perm = list(range(L))
        for dst, src in zip(movable, rng.permutation(movable).tolist()):
            perm[dst] = src
        shuffled = [seq[i] for i in perm]
        distance = sum(1 for x in ndiff(shuffled, seq) if x[0] != ' ')
        similarity = 1 - distance / L
        if similarity <= MAX_SIMILARITY:
            return ''.join(shuffled), perm
        if similarity < best_similarity:
            best_similarity, best = similarity, perm
    return ''.join(seq[i] for i in best), best


def decoy_batch(raw, seq_offsets, residue_mass, perm, nterm, cterm, max_fragment_charge, tol: float,
                unit: str, device='cuda') -> dict:
    """``asl_decoy_batch`` on a ``PackedSpectra`` of raw peaks: the decoy peaks (``mz``, ``intensity``,
    ``src``, ``charge``: decoy order) and the annotation found (``ann_type`` 0 none / 1 a / 2 b / 3 p /
    4 y, ``ann_n``, ``ann_z``, ``ann_loss``: raw order), torch tensors on ``device``."""
    import torch
    if unit not in ('Da', 'ppm'):
        raise ValueError(f"unit = {unit!r}: 'Da' or 'ppm'")
    r = raw.to(device).contiguous()
    dev = r.mz.device
    P = int(r.mz.numel())
    f = lambda a, dt: np.ascontiguousarray(a, dt)
    seq_offsets, perm, zmax = f(seq_offsets, np.int32), f(perm, np.int32), f(max_fragment_charge, np.int32)
    residue_mass, nterm, cterm = f(residue_mass, np.float64), f(nterm, np.float64), f(cterm, np.float64)
    if not (len(seq_offsets) == r.n + 1 and len(nterm) == len(cterm) == len(zmax) == r.n and
            len(residue_mass) == len(perm) and (r.n == 0 or len(perm) >= int(seq_offsets[-1]))):
        raise ValueError('decoy_batch: array lengths do not match the spectra')
    out = dict(mz=torch.zeros(P, dtype=torch.float32, device=dev),
               intensity=torch.zeros(P, dtype=torch.float32, device=dev),
               src=torch.zeros(P, dtype=torch.int32, device=dev))
    for k in ('charge', 'ann_type', 'ann_n', 'ann_z', 'ann_loss'):
        out[k] = torch.zeros(P, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().asl_decoy_batch(
        C.byref(_lib.peaks_struct(r)), _lib.ptr(seq_offsets), _lib.ptr(residue_mass), _lib.ptr(perm),
        _lib.ptr(nterm), _lib.ptr(cterm), _lib.ptr(zmax), float(tol), 0 if unit == 'Da' else 1,
        *[_lib.ptr(out[k]) for k in ('mz', 'intensity', 'src', 'charge', 'ann_type', 'ann_n', 'ann_z',
                                     'ann_loss')]))
    return out


def default_fragment_charge(precursor_charge: int) -> int:
    """spectrum_utils' default for ``annotate_proforma``: up to one below the precursor charge."""
    return max(1, int(precursor_charge) - 1)


def shuffle_and_reposition_batch(raw, peptides: Sequence[str], tol: float, unit: str = 'ppm', seed: int = 1234,
                                 device='cuda', modification_masses: Optional[Dict[str, float]] = None):
    """Decoys of a ``PackedSpectra`` of RAW library spectra with the peptides ``peptides[i]``.
    Returns ``(decoy PackedSpectra on device, decoy peptide strings, annotation)``: the decoy pack has
    the targets' precursors, per-peak fragment charges from the annotation and identifiers
    ``'DECOY_' + id``; ``annotation`` holds ``type`` / ``n`` / ``z`` / ``loss`` per RAW target peak (torch,
    on ``device``; ``z`` is the targets' new charge column) and ``perm`` per spectrum."""
    from .packed import PackedSpectra
    if len(peptides) != raw.n:
        raise ValueError(f'{len(peptides)} peptides for {raw.n} spectra')
    ids = raw.identifiers if raw.identifiers is not None else list(range(raw.n))
    pz = raw.precursor_charge.cpu().numpy()
    seq_off, masses, perms, nterm, cterm, zmax, names = [0], [], [], [], [], [], []
    for i, text in enumerate(peptides):
        pep = parse_peptide(text, modification_masses, ids[i])
        if len(pep.sequence) < 2:
            raise ValueError(f'peptide {text!r} of spectrum {ids[i]!r}: a decoy needs 2 residues or more')
        _, perm = shuffle(pep.sequence, peptide_rng(seed, text, pz[i]))
        masses.append(pep.masses)
        perms.append(np.asarray(perm, np.int32))
        seq_off.append(seq_off[-1] + len(perm))
        nterm.append(pep.nterm)
        cterm.append(pep.cterm)
        zmax.append(default_fragment_charge(pz[i]))
        names.append(str(pep.permuted(perm)))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    out = decoy_batch(raw, seq_off, cat(masses, np.float64), cat(perms, np.int32), nterm, cterm, zmax, tol,
                      unit, device)
    r = raw.to(device)
    decoy = PackedSpectra(r.offsets, out['mz'], out['intensity'], out['charge'], r.precursor_mz,
                          r.precursor_charge, identifiers=['DECOY_' + str(i) for i in ids])
    annotation = dict(type=out['ann_type'], n=out['ann_n'], z=out['ann_z'], loss=out['ann_loss'],
                      src=out['src'], perm=perms)
    return decoy, names, annotation


class LibrarySpectrum:
    """A library spectrum as the packed store reads it (library_store.py): raw peaks ascending in m/z
    with their fragment charges (``charge``, 0 = not annotated)."""

    def __init__(self, identifier, precursor_mz, precursor_charge, mz, intensity, charge, peptide,
                 is_decoy, retention_time=None):
        self.identifier = identifier
        self.precursor_mz = precursor_mz
        self.precursor_charge = precursor_charge
        self.mz = mz
        self.intensity = intensity
        self.charge = charge
        self.annotation = None
        self.peptide = peptide
        self.is_decoy = is_decoy
        self.retention_time = retention_time


def shuffle_and_reposition(spectrum, tol: float = 0.02, unit: str = 'ppm', seed: int = 1234, device='cuda',
                           modification_masses: Optional[Dict[str, float]] = None) -> LibrarySpectrum:
    """The reference's call shape: one spectrum object (``identifier``, ``precursor_mz``,
    ``precursor_charge``, ``mz``, ``intensity``, ``peptide``) in, its decoy out: identifier ``'DECOY_' +
    id``, the same precursor, ``is_decoy = True``, the shuffled ``peptide``."""
    from .library_store import pack_raw
    raw = pack_raw([spectrum])
    decoy, names, _ = shuffle_and_reposition_batch(raw, [spectrum.peptide], tol, unit, seed, device,
                                                   modification_masses)
    _, mz, it, chg, _, _ = decoy.numpy()
    return LibrarySpectrum('DECOY_' + str(spectrum.identifier), spectrum.precursor_mz,
                           spectrum.precursor_charge, mz, it, chg, names[0], True,
                           getattr(spectrum, 'retention_time', None))
