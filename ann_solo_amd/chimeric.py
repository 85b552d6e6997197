"""Chimeric spectra: what is left of a query spectrum once its identification has taken its peaks.

One HIP kernel (``asl_deplete_batch``, csrc/deplete.hip) removes from every query of a batch the peaks its
winning library spectrum explains -- a peak is explained when the shifted dot product's own window test could
have paired it with a library peak -- and re-normalises the rest as ``asl_process_batch`` normalises, so a
residue is a processed spectrum like any other. The definition is written down in include/annsolo_mi.h and
DESIGN.md 3 "Chimeric search"; tests/deplete_ref.py restates it in numpy. ``SpectralLibrary.search_packed``
searches the valid residues as one more cascade level with ``Config.chimeric_search``.
"""
import ctypes as C

import numpy as np

from . import _lib
from .packed import PackedSpectra

BATCH = 32768
MAX_PEAKS = 4096            # csrc/deplete.hip: DP_MAXN
KEYS = ('mz', 'intensity', 'src', 'count', 'valid', 'kept_energy')


def deplete_batch(queries, library, lib_rows, tol: float, flags: int, min_peaks: int, min_mz_range: float,
                  device='cuda') -> dict:
    """``asl_deplete_batch``: query ``s`` of the ``PackedSpectra`` ``queries`` against row ``lib_rows[s]`` of
    ``library`` (< 0: skipped). ``tol`` is ``fragment_mz_tolerance`` and ``flags`` the search's score flag word
    (``spectrum_match.score_flags``). Torch tensors on ``device``: ``mz``, ``intensity`` (float32) and ``src``
    (int32, the kept peak's index in its query), ``[n, stride]`` with ``stride`` the largest peak count of a
    query, zero beyond ``count``; ``count`` (int32), ``valid`` (uint8) and ``kept_energy`` (float32), ``[n]``."""
    import torch
    q = queries.to(device).contiguous()
    lib = library.to(device).contiguous()
    dev = q.mz.device
    rows = torch.as_tensor(np.asarray(lib_rows) if not hasattr(lib_rows, 'data_ptr') else lib_rows)
    rows = rows.to(device=dev, dtype=torch.int64).contiguous()
    n = q.n
    if rows.ndim != 1 or rows.numel() != n:
        raise ValueError(f'deplete_batch: {tuple(rows.shape)} library rows for {n} queries')
    stride = q.max_peaks()
    out = {'mz': torch.zeros((n, stride), dtype=torch.float32, device=dev),
           'intensity': torch.zeros((n, stride), dtype=torch.float32, device=dev),
           'src': torch.zeros((n, stride), dtype=torch.int32, device=dev),
           'count': torch.zeros(n, dtype=torch.int32, device=dev),
           'valid': torch.zeros(n, dtype=torch.uint8, device=dev),
           'kept_energy': torch.zeros(n, dtype=torch.float32, device=dev)}
    L = _lib.lib()
    if not hasattr(L, 'asl_deplete_batch'):
        raise _lib.AnnSoloMiError('libannsolo_mi has no asl_deplete_batch (an older library given by ASL_LIB_PATH)')
    _lib.check(L.asl_deplete_batch(C.byref(_lib.peaks_struct(q)), C.byref(_lib.peaks_struct(lib)), _lib.ptr(rows),
                                   float(tol), int(flags), int(min_peaks), float(min_mz_range), stride,
                                   *[_lib.ptr(out[k]) for k in KEYS]))
    return out


def pack_residues(out: dict, queries: PackedSpectra):
    """The valid rows of a ``deplete_batch`` result as a ``PackedSpectra`` (torch ops on the result's device, as
    ``pack_queries`` packs after ``asl_process_batch``): the queries' own precursor m/z and charge, no peak
    annotation. Returns ``(pack, rows)``, ``rows`` (int64 tensor) the batch rows the spectra come from."""
    import torch
    dev = out['count'].device
    rows = torch.nonzero(out['valid'] != 0).flatten()
    cnt = out['count'][rows].to(torch.int64)
    off = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(cnt, 0)
    stride = out['mz'].shape[1]
    mask = torch.arange(stride, device=dev)[None, :] < cnt[:, None]
    mz, inten = out['mz'][rows][mask], out['intensity'][rows][mask]      # (row-major: the peaks stay in order)
    q = queries.to(dev)
    ids = None if queries.identifiers is None else [queries.identifiers[int(r)] for r in rows.cpu()]
    pack = PackedSpectra(off.to(torch.int32), mz, inten, torch.zeros(mz.numel(), dtype=torch.uint8, device=dev),
                         q.precursor_mz[rows], q.precursor_charge[rows], identifiers=ids)
    return pack, rows


def residues(queries, library, lib_rows, tol: float, flags: int, min_peaks: int, min_mz_range: float,
             device='cuda'):
    """``deplete_batch`` in batches of 32 768 and the packing of its valid rows: ``(pack, rows, kept_energy)``
    -- the residue spectra as a ``PackedSpectra`` on ``device``, the rows of ``queries`` they come from (int64
    numpy) and, for EVERY query, the share of squared intensity its library row leaves unexplained (float32
    numpy, ``[queries.n]``; 0 where ``lib_rows`` is negative)."""
    import torch
    from .library_store import concat_packs
    rows_np = np.asarray(lib_rows.cpu() if hasattr(lib_rows, 'cpu') else lib_rows, np.int64)
    packs, src, energy = [], [], []
    for b0 in range(0, queries.n, BATCH):
        sel = torch.arange(b0, min(b0 + BATCH, queries.n))
        q = queries if len(sel) == queries.n else queries.select(sel)
        out = deplete_batch(q, library, rows_np[b0:b0 + BATCH], tol, flags, min_peaks, min_mz_range, device)
        pack, rows = pack_residues(out, q)
        packs.append(pack)
        src.append(rows.cpu().numpy().astype(np.int64) + b0)
        energy.append(out['kept_energy'].cpu().numpy())
    if not packs:
        dev = torch.device(device)
        z = lambda dt: torch.zeros(0, dtype=dt, device=dev)
        empty = PackedSpectra(torch.zeros(1, dtype=torch.int32, device=dev), z(torch.float32), z(torch.float32),
                              z(torch.uint8), z(torch.float64), z(torch.int32))
        return empty, np.zeros(0, np.int64), np.zeros(0, np.float32)
    return concat_packs(packs), np.concatenate(src), np.concatenate(energy)
