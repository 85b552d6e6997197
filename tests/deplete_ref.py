"""The depletion of a query spectrum by its winning library spectrum (include/annsolo_mi.h:
asl_deplete_batch, DESIGN.md 3 "Chimeric search"), restated in numpy one spectrum at a time: the yardstick
of csrc/deplete.hip, bit for bit, and the stand-in for ``chimeric.deplete_batch`` on a machine without a GPU.

Every comparison is an fp64 numpy operation, one IEEE operation each (numpy does not contract a multiply
and an add). There is no cursor and no search: every (query peak, library peak, shift) triple is tested.
The norm is process.hip's: an ascending float32 chain of TRUE fused multiply-adds (one rounding per step)
-- libm's ``fmaf`` through ctypes, or ``math.fma`` on exactly representable doubles where Python has it
(a float32 product is exact in double, so fma in double followed by one rounding to float32 would round
twice: libm's is preferred and ``math.fma`` is only used through the exact two-step below)."""
import ctypes
import ctypes.util
import math

import numpy as np

SCORE_SHIFT, SCORE_FRAGMENT_PPM = 1, 2
MAX_PEAKS = 4096


def _libm_fmaf():
    name = ctypes.util.find_library('m')
    for cand in (name, 'libm.so.6'):
        if not cand:
            continue
        try:
            f = ctypes.CDLL(cand).fmaf
        except (OSError, AttributeError):
            continue
        f.restype = ctypes.c_float
        f.argtypes = [ctypes.c_float] * 3
        return lambda a, b, c: np.float32(f(float(a), float(b), float(c)))
    return None


def _exact_fmaf():
    """float32 fma without libm: a * b is exact in double (24 + 24 bits); the sum with c is rounded to float32
    ONCE by rounding to odd in double first (``math.fma`` gives the exactly rounded double of a * b + c; the
    sticky bit is recovered from the residual, so the second rounding cannot double-round)."""
    if not hasattr(math, 'fma'):
        return None

    def f(a, b, c):
        a, b, c = float(a), float(b), float(c)
        p = a * b                                   # exact
        s = p + c                                   # rounded double
        if math.isinf(s) or math.isnan(s):
            return np.float32(s)
        bb = s - p
        err = (p - (s - bb)) + (c - bb)             # TwoSum: s + err == p + c exactly
        if err != 0.0:
            m = np.array([s], np.float64).view(np.int64)
            if (m[0] & 1) == 0:                     # round to odd: an inexact even mantissa moves toward err
                s = float(np.nextafter(s, math.inf if err > 0 else -math.inf))
        return np.float32(s)
    return f


fmaf = _libm_fmaf() or _exact_fmaf()
if fmaf is None:        # (never the double-rounded np.float32(a * a + acc))
    raise ImportError('deplete_ref: neither libm fmaf nor math.fma is available')


def flags_of(shift, unit='Da'):
    return (SCORE_SHIFT if shift else 0) | (SCORE_FRAGMENT_PPM if unit == 'ppm' else 0)


def shifts_of(q_pmz, l_pmz, z, tol, flags):
    """(num_shifts, pmd): step 1 of the contract."""
    if flags & ~(SCORE_SHIFT | SCORE_FRAGMENT_PPM):
        raise ValueError('flag bits other than SHIFT | FRAGMENT_PPM')
    t = np.float64(tol)
    pmd = (np.float64(q_pmz) - np.float64(l_pmz)) * np.float64(int(z))
    gate_at = (t * np.float64(1e-6)) * np.float64(q_pmz) if flags & SCORE_FRAGMENT_PPM else t
    gate = bool(np.abs(pmd) >= gate_at)
    return (int(z) + 1 if (flags & SCORE_SHIFT and gate) else 1), pmd


def explained(q_mz, q_pmz, l_mz, l_chg, l_pmz, z, tol, flags, chunk=1 << 22):
    """Boolean per query peak: step 2, every (i, j, c)."""
    qm = np.asarray(q_mz, np.float32).astype(np.float64)
    lm = np.asarray(l_mz, np.float32).astype(np.float64)
    chg = (np.zeros(len(lm), np.int64) if l_chg is None else np.asarray(l_chg).astype(np.int64))
    S, pmd = shifts_of(q_pmz, l_pmz, z, tol, flags)
    t = np.float64(tol)
    tl = (t * np.float64(1e-6)) * qm if flags & SCORE_FRAGMENT_PPM else np.full(len(qm), t)
    out = np.zeros(len(qm), bool)
    if len(qm) == 0 or len(lm) == 0:
        return out
    step = max(1, chunk // len(lm))
    for c in range(max(S, 0)):
        md = np.float64(0.0) if c == 0 else pmd / np.float64(c)
        x = lm + md
        ok_j = np.ones(len(lm), bool) if c == 0 else ((chg == c) | (chg == 0))
        if not ok_j.any():
            continue
        xs = x[ok_j]
        for a in range(0, len(qm), step):
            sl = slice(a, a + step)
            with np.errstate(invalid='ignore'):
                hit = np.abs(qm[sl, None] - xs[None, :]) <= tl[sl, None]
            out[sl] |= hit.any(axis=1)
    return out


def deplete_one(q_mz, q_int, q_pmz, l_mz, l_chg, l_pmz, z, tol, flags, min_peaks, min_mz_range):
    """One SSM: dict(mz, intensity, src, count, valid, energy) -- arrays of the kept peaks only."""
    q_mz, q_int = np.asarray(q_mz, np.float32), np.asarray(q_int, np.float32)
    keep = ~explained(q_mz, q_pmz, l_mz, l_chg, l_pmz, z, tol, flags)
    src = np.nonzero(keep)[0].astype(np.int32)
    mz, v = q_mz[src], q_int[src]
    acc = np.float32(0.0)
    for x in v:
        acc = fmaf(x, x, acc)
    nrm = np.sqrt(acc, dtype=np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        inten = (v / nrm).astype(np.float32)
    n = len(src)
    valid = bool(n >= min_peaks and n > 0 and np.float64(np.float32(mz[-1] - mz[0])) >= np.float64(min_mz_range))
    return dict(mz=mz, intensity=inten, src=src, count=n, valid=valid, energy=acc)


def deplete_batch(queries, library, lib_rows, tol, flags, min_peaks, min_mz_range, stride=None):
    """The batch, on packed numpy tuples (offsets, mz, intensity, charge or None, precursor_mz,
    precursor_charge): dict of numpy arrays shaped as ``asl_deplete_batch`` writes them (``mz``, ``intensity``,
    ``src`` [n, stride] zero padded; ``count``, ``valid``, ``kept_energy`` [n]). Raises ValueError where the
    entry returns an error."""
    if not np.float64(tol) >= 0.0:
        raise ValueError('negative or NaN tolerance')
    shifts_of(0.0, 0.0, 1, tol, flags)
    qo, qmz, qit, _, qp, _ = queries
    lo, lmz, _, lch, lp, lz = library
    n = len(qo) - 1
    counts = np.diff(np.asarray(qo, np.int64))
    if n and counts.max() > MAX_PEAKS:
        raise OverflowError('more than 4096 peaks')
    need = int(counts.max()) if n else 0
    stride = need if stride is None else int(stride)
    if stride < need:
        raise OverflowError('out_stride below the largest query')
    out = dict(mz=np.zeros((n, stride), np.float32), intensity=np.zeros((n, stride), np.float32),
               src=np.zeros((n, stride), np.int32), count=np.zeros(n, np.int32), valid=np.zeros(n, np.uint8),
               kept_energy=np.zeros(n, np.float32))
    rows = np.asarray(lib_rows, np.int64)
    if (rows >= len(lo) - 1).any():
        raise ValueError('a row beyond the library')
    for s in range(n):
        r = int(rows[s])
        if r < 0:
            continue
        if lo[r + 1] - lo[r] > MAX_PEAKS:
            raise OverflowError('more than 4096 peaks')
    for s in range(n):
        r = int(rows[s])
        if r < 0:
            continue
        a, b = slice(int(qo[s]), int(qo[s + 1])), slice(int(lo[r]), int(lo[r + 1]))
        one = deplete_one(qmz[a], qit[a], qp[s], lmz[b], None if lch is None else lch[b], lp[r], int(lz[r]), tol,
                          flags, min_peaks, min_mz_range)
        k = one['count']
        out['mz'][s, :k], out['intensity'][s, :k], out['src'][s, :k] = one['mz'], one['intensity'], one['src']
        out['count'][s], out['valid'][s], out['kept_energy'][s] = k, one['valid'], one['energy']
    return out


def torch_deplete_batch(queries, library, lib_rows, tol, flags, min_peaks, min_mz_range, device='cpu'):
    """``ann_solo_amd.chimeric.deplete_batch`` answered by the reference: ``PackedSpectra`` in, a dict of CPU
    torch tensors out (the tests monkeypatch it in where there is no GPU)."""
    import torch
    rows = lib_rows.cpu().numpy() if hasattr(lib_rows, 'cpu') else np.asarray(lib_rows)
    out = deplete_batch(queries.numpy(), library.numpy(), rows, tol, flags, min_peaks, min_mz_range,
                        stride=queries.max_peaks())
    return {k: torch.from_numpy(v) for k, v in out.items()}
