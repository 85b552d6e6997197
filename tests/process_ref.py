"""The numpy formulation of process_spectrum (reference spectrum.py:57-119 over spectrum_utils
0.3.x -- un-vendored, PARITY UNPINNED), written the way spectrum_utils' array code reads
(boolean masks, argsort). Test-side helper: the definition the oracle's restatement
(oracle/asl_oracle.c: orc_process_spectrum) and, through it, the device kernel are held to."""
import numpy as np


def numpy_process(mz, it, pmz, pz, min_mz=11, max_mz=2010, remove_precursor=False, rp_tol=0.0,
                  min_intensity=0.01, max_peaks=50, scaling='rank', min_peaks=10,
                  min_mz_range=250.0, resolution=None):
    def valid(m):                                            # spectrum.py:13-36
        return len(m) >= min_peaks and len(m) > 0 and float(m[-1] - m[0]) >= min_mz_range
    idx = np.arange(len(mz))
    keep = (mz.astype(np.float64) >= min_mz) & (mz.astype(np.float64) <= max_mz)
    mz, it, idx = mz[keep], it[keep], idx[keep]
    if not valid(mz):
        return False, None, None, None
    if resolution is not None:                               # spectrum.py:84-85 round(d, 'sum')
        rmz = np.round(mz.astype(np.float64), resolution).astype(np.float32)
        uniq, first, inv = np.unique(rmz, return_index=True, return_inverse=True)
        it_sum = np.zeros(len(uniq), np.float32)
        best = first.copy()
        for j in range(len(rmz)):                            # sequential float32 sum, first argmax
            g = inv[j]
            it_sum[g] = np.float32(it_sum[g] + it[j])
            if it[j] > it[best[g]]:
                best[g] = j
        mz, it, idx = uniq, it_sum, idx[best]
        if not valid(mz):
            return False, None, None, None
    if remove_precursor:
        neutral = (pmz - 1.0072766) * pz
        rm = np.array([(neutral + iso) / c + 1.0072766 for c in range(pz, 0, -1)
                       for iso in range(3)])
        far = (np.abs(mz.astype(np.float64)[:, None] - rm[None, :]) > rp_tol).all(1)
        mz, it, idx = mz[far], it[far], idx[far]
        if not valid(mz):
            return False, None, None, None
    order = np.argsort(it, kind='stable')[::-1]              # descending; ties: later peak first
    top = order[:max_peaks]
    top = top[it[top].astype(np.float64) > min_intensity * float(it.max())]
    sel = np.sort(top)
    if not valid(mz[sel]):
        return False, None, None, None
    if scaling == 'rank':
        val = np.zeros(len(mz), np.float32)
        val[top] = max_peaks - np.arange(len(top), dtype=np.float32)
        val = val[sel]
    elif scaling == 'sqrt':
        val = np.sqrt(it[sel])
    else:
        val = it[sel].copy()
    acc = np.float32(0)
    for v in val:                                            # canonical ascending fp32 chain
        acc = np.float32(np.float64(v) * np.float64(v) + np.float64(acc))
    return True, mz[sel], val / np.sqrt(acc), idx[sel]
