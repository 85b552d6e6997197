"""Modification site localisation for open-search matches: which residue of the library peptide do the
query's own peaks put the unknown mass on?

One HIP kernel (``asl_localize_batch``, csrc/localize.hip) scores every site of every SSM of a batch; the
definition -- plain and shifted b / y fragments, the most intense peak inside the tolerance, sequential
fp64 sums per site -- is written down in include/annsolo_mi.h and DESIGN.md 3 "Localisation", and
tests/localize_ref.py restates it in numpy. The tolerance in ppm is of the THEORETICAL fragment m/z, as for
the decoys, not of the query peak as in the shifted dot product. Sites are 0-based residue indices,
N-terminal residue first.
"""
import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib
from .decoy_generator import default_fragment_charge, parse_peptide

BATCH = 32768
MAX_RESIDUES = 128          # csrc/fragments.hpp: DC_MAXL
MAX_FRAGMENT_CHARGE = 8     # DC_MAXZ
SITE_KEYS = ('site_score', 'site_count')
SSM_KEYS = ('best_lo', 'best_hi', 'n_best', 'best_count', 'best_score', 'runner_score', 'none_score')


def localize_batch(spectra, seq_offsets, residue_mass, nterm, cterm, max_fragment_charge, delta, tol: float,
                   unit: str, device='cuda') -> dict:
    """``asl_localize_batch`` on a ``PackedSpectra`` of query spectra (peaks ascending in m/z), one SSM
    per spectrum: torch tensors on ``device`` -- per site, in the peptides' CSR layout, ``site_score``
    (float64) and ``site_count`` (int32); per SSM ``best_lo``, ``best_hi``, ``n_best``, ``best_count``
    (int32), ``best_score``, ``runner_score``, ``none_score`` (float64). Array lengths that do not match
    the spectra are a ``ValueError`` before any device call."""
    import torch
    if unit not in ('Da', 'ppm'):
        raise ValueError(f"unit = {unit!r}: 'Da' or 'ppm'")
    f = lambda a, dt: np.ascontiguousarray(a, dt)
    seq_offsets, zmax = f(seq_offsets, np.int32), f(max_fragment_charge, np.int32)
    residue_mass, nterm, cterm, delta = (f(a, np.float64) for a in (residue_mass, nterm, cterm, delta))
    n = spectra.n
    if not (seq_offsets.ndim == 1 and len(seq_offsets) == n + 1 and
            len(nterm) == len(cterm) == len(zmax) == len(delta) == n and
            (n == 0 or len(residue_mass) >= int(seq_offsets[-1]))):
        raise ValueError('localize_batch: array lengths do not match the spectra')
    r = spectra.to(device).contiguous()
    dev = r.mz.device
    R = int(seq_offsets[-1]) if n else 0
    out = {}
    for k in SITE_KEYS + SSM_KEYS:
        out[k] = torch.zeros(R if k in SITE_KEYS else n, device=dev,
                             dtype=torch.float64 if k.endswith('score') else torch.int32)
    _lib.check(_lib.lib().asl_localize_batch(
        C.byref(_lib.peaks_struct(r)), _lib.ptr(seq_offsets), _lib.ptr(residue_mass), _lib.ptr(nterm),
        _lib.ptr(cterm), _lib.ptr(zmax), _lib.ptr(delta), float(tol), 0 if unit == 'Da' else 1,
        *[_lib.ptr(out[k]) for k in SITE_KEYS + SSM_KEYS]))
    return out


def localize_peptides(spectra, peptides: Sequence[str], delta, tol: float, unit: str = 'Da', device='cuda',
                      modification_masses: Optional[Dict[str, float]] = None) -> dict:
    """``localize_batch`` for peptide strings (``decoy_generator.parse_peptide``: the peptides' own
    modifications are folded into their residues): spectrum ``i`` of ``spectra`` against ``peptides[i]``
    carrying ``delta[i]``. The largest fragment charge is ``default_fragment_charge`` of the spectrum's
    precursor charge, clipped to 8. Also returns ``seq_offsets`` (numpy) to slice the per-site arrays."""
    if len(peptides) != spectra.n:
        raise ValueError(f'{len(peptides)} peptides for {spectra.n} spectra')
    ids = spectra.identifiers if spectra.identifiers is not None else list(range(spectra.n))
    peps = [parse_peptide(text, modification_masses, ids[i]) for i, text in enumerate(peptides)]
    arrays = peptide_arrays(peps, spectra.precursor_charge.cpu().numpy())
    out = localize_batch(spectra, *arrays, delta, tol, unit, device)
    out['seq_offsets'] = arrays[0]
    return out


def peptide_arrays(peptides, precursor_charges) -> tuple:
    """``(seq_offsets, residue_mass, nterm, cterm, max_fragment_charge)`` of parsed peptides
    (``decoy_generator.Peptide``) for ``localize_batch``."""
    seq_off = np.zeros(len(peptides) + 1, np.int32)
    seq_off[1:] = np.cumsum([len(p.sequence) for p in peptides])
    mass = np.concatenate([p.masses for p in peptides]) if len(peptides) else np.zeros(0, np.float64)
    zmax = [min(default_fragment_charge(z), MAX_FRAGMENT_CHARGE) for z in precursor_charges]
    return (seq_off, mass.astype(np.float64), np.asarray([p.nterm for p in peptides], np.float64),
            np.asarray([p.cterm for p in peptides], np.float64), np.asarray(zmax, np.int32))
