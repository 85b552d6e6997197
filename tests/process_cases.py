"""Named deterministic spectra for the preprocessing kernel (csrc/process.hip), its oracle
restatement (oracle/asl_oracle.c: orc_process_spectrum) and the numpy definition
(process_ref.numpy_process): the sort sizes, ties at the cut-off, threshold and validity
equalities, long merge runs, precursor removal at its tolerance and bad intensities that
random spectra do not reach. Pure numpy; test-side helper (no GPU, no oracle).

``CASES`` is a list of ``Case(name, mz f32, intensity f32, charge u8, precursor_mz,
precursor_charge, cfg, exp)``. ``cfg`` holds numpy_process' keyword arguments. ``exp`` says what
the case is built to hit, derived from the construction and never from a run of the code:
``valid``, and where they are known ``count`` (survivors), ``src`` (their source indices,
ascending) and ``mz`` (their m/z after rounding)."""
from collections import namedtuple

import numpy as np

Case = namedtuple('Case', 'name mz intensity charge precursor_mz precursor_charge cfg exp')

CASES = []
F32 = np.float32
NAN_POS = np.array([0x7FC00000], np.uint32).view(F32)[0]
NAN_NEG = np.array([0xFFC00000], np.uint32).view(F32)[0]     # what x86 gives for 0.0f / 0.0f
ADDUCT = 1.0072766


def _add(name, mz, it, cfg, valid, count=None, src=None, out_mz=None, pmz=700.0, pz=2, seed=0):
    mz, it = np.ascontiguousarray(mz, F32), np.ascontiguousarray(it, F32)
    assert len(mz) == len(it) <= 4096 and (np.diff(mz) >= 0).all(), name
    assert name not in [c.name for c in CASES], name
    chg = np.random.default_rng(1000 + seed).integers(0, 4, len(mz)).astype(np.uint8)
    exp = dict(valid=bool(valid))
    if src is not None:
        src = np.asarray(src, np.int64)
        count = len(src)
        exp['src'] = src
    if count is not None:
        exp['count'] = int(count)
    if out_mz is not None:
        exp['mz'] = np.asarray(out_mz, F32)
    assert valid or not (count or src is not None), name
    CASES.append(Case(name, mz, it, chg, float(pmz), int(pz), dict(cfg), exp))


def cfg_key(cfg):
    return tuple(sorted(cfg.items(), key=lambda kv: kv[0]))


def oracle_args(cfg):
    """``cfg`` as the keyword arguments of oracle_py.process_spectrum."""
    kw = dict(cfg)
    if 'rp_tol' in kw:
        kw['remove_precursor_tolerance'] = kw.pop('rp_tol')
    return kw


def config_attrs(cfg):
    """``cfg`` under the reference's config names (what spectrum.process_spectra reads for a query)."""
    kw = oracle_args(cfg)
    if 'max_peaks' in kw:
        kw['max_peaks_used'] = kw.pop('max_peaks')
    return kw


def _grid(n, lo=100.0, hi=1900.0):
    return np.linspace(lo, hi, n).astype(F32)


def _flat(rng, n):
    """Distinct intensities in [1, 2): all of them far above 1 % of the base peak."""
    it = rng.uniform(1.0, 2.0, n).astype(F32)
    assert len(np.unique(it)) == n
    return it


# ---------------------------------------------------------------------------- 1. sort sizes
# The kernel sorts 256 / 1024 / 4096 keys by the RAW peak count. m/z uniform in [5, 2100]: some
# peaks fall outside [11, 2010], so the in-range count is below the raw count that picks the sort.
def _sort_sizes():
    scalings = ['rank', 'sqrt', None]
    sizes = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096]
    for a, n in enumerate(sizes):
        rng = np.random.default_rng(100 + n)
        mz = np.sort(rng.uniform(5, 2100, n)).astype(F32)
        it = rng.lognormal(0, 1.5, n).astype(F32)
        inr = np.nonzero((mz.astype(np.float64) >= 11) & (mz.astype(np.float64) <= 2010))[0]
        assert n == 1 or 0 < len(inr) < n
        if n == 1:                                          # a lone peak outside the window tests nothing
            mz[0] = F32(700.25)
            inr = np.array([0])
        assert (it[inr] == it[inr].max()).sum() == 1         # one base peak: max_peaks = 1 keeps it
        above = int((it[inr].astype(np.float64) > 0.01 * float(it[inr].max())).sum())
        for b, mp in enumerate([1, 50, 255, 256]):
            cfg = dict(max_peaks=mp, min_peaks=1, min_mz_range=0.0, scaling=scalings[(a // 3 + b) % 3])
            src = [inr[np.argmax(it[inr])]] if mp == 1 else None
            _add(f'sort_n{n}_mp{mp}', mz, it, cfg, True, count=min(mp, above), src=src, seed=n)


# ---------------------------------------------------------------------------- 2. cut-off ties
def _ties():
    # (a) all equal: (intensity desc, index desc) keeps the LAST max_peaks peaks
    _add('tie_all_equal', _grid(300), np.ones(300), dict(), True, src=np.arange(250, 300))
    # (b) ten levels of 30 peaks, interleaved along m/z; the cut at 50 falls inside level 9: all of
    # level 10 and the 20 LAST peaks of level 9
    level = (np.arange(300) % 10 + 1).astype(F32)
    l10, l9 = np.nonzero(level == 10)[0], np.nonzero(level == 9)[0]
    _add('tie_levels', _grid(300), level, dict(max_peaks=50), True,
         src=np.sort(np.concatenate([l10, l9[-20:]])))
    # (c) as (a) over merged heads (the 6.02 m/z grid rounds to 300 distinct integers)
    g = _grid(300)
    _add('tie_all_equal_rounded', g, np.ones(300), dict(resolution=0), True,
         src=np.arange(250, 300), out_mz=np.round(g[250:].astype(np.float64)))


# ---------------------------------------------------------------------------- 3. threshold equality
def _threshold():
    it = np.full(42, 8.0, F32)
    it[20] = 4.0                                            # == 0.5 * base peak: strict '>' drops it
    it[21] = np.nextafter(F32(4.0), F32(np.inf))
    _add('thresh_equal', _grid(42), it, dict(min_intensity=0.5), True,
         src=np.delete(np.arange(42), 20))
    rng = np.random.default_rng(31)
    it = _flat(rng, 40)
    it[[3, 17, 39]] = 0.0
    # tiny but normal numbers are kept (no denormal: whether the host reference sees one depends on
    # the FTZ / DAZ mode that libraries loaded earlier into the test process leave behind)
    it[5], it[30] = 1e-30, 2e-38
    _add('thresh_zero', _grid(40), it, dict(min_intensity=0.0), True,
         src=np.delete(np.arange(40), [3, 17, 39]))


# ---------------------------------------------------------------------------- 4. validity edges
# min_peaks = 10 survivors are valid, 9 are not -- with the count dropping at one checkpoint only.
def _validity():
    rng = np.random.default_rng(41)
    for k, ok in ((10, True), (9, False)):
        # after the range filter: k in-range peaks, three below and three above the window
        mz = np.concatenate([[5.0, 8.0, 10.9], _grid(k), [2010.5, 2050.0, 2099.0]])
        _add(f'valid_range_{k}', mz, _flat(rng, k + 6), dict(), ok,
             src=np.arange(3, 3 + k) if ok else None)
        # after the merge: k + 1 peaks, 503 and 504 both round to 500 at resolution -1
        base = _grid(k - 1, 100.0, 1900.0)
        mz = np.sort(np.concatenate([base, [503.0, 504.0]])).astype(F32)
        assert len(np.unique(np.round(mz.astype(np.float64), -1))) == k
        it = _flat(rng, k + 1)
        a = int(np.searchsorted(mz, F32(503.0)))
        it[a], it[a + 1] = 1.25, 1.5                        # the later one carries the annotation
        _add(f'valid_merge_{k}', mz, it, dict(resolution=-1), ok,
             src=np.delete(np.arange(k + 1), a) if ok else None)
        # after precursor removal: k + 1 peaks, one on the precursor (z = 1: 510, 511, 512)
        mz = np.sort(np.concatenate([_grid(k), [510.0]])).astype(F32)
        a = int(np.searchsorted(mz, F32(510.0)))
        assert len(np.unique(mz)) == k + 1
        _add(f'valid_precursor_{k}', mz, _flat(rng, k + 1), dict(remove_precursor=True, rp_tol=0.1),
             ok, src=np.delete(np.arange(k + 1), a) if ok else None, pmz=510.0, pz=1)
        # after the intensity filter: k + 1 peaks, one below 1 % of the base peak
        it = _flat(rng, k + 1)
        it[4] = 0.001
        _add(f'valid_intensity_{k}', _grid(k + 1), it, dict(), ok,
             src=np.delete(np.arange(k + 1), 4) if ok else None)
    # the m/z span: fp32 difference against min_mz_range = 250 in double
    for name, last, ok in (('valid_span_250', F32(350.0), True),
                           ('valid_span_below_250', np.nextafter(F32(350.0), F32(0)), False)):
        mz = _grid(12, 100.0, 350.0)
        mz[-1] = last
        _add(name, mz, _flat(rng, 12), dict(), ok, src=np.arange(12) if ok else None)
    _add('all_below_min_mz', np.linspace(1, 10.9, 30), _flat(rng, 30), dict(), False)
    _add('all_above_max_mz', np.linspace(2010.1, 2500, 30), _flat(rng, 30), dict(), False)
    _add('empty', np.zeros(0), np.zeros(0), dict(), False)


# ---------------------------------------------------------------------------- 5. merge
MERGE = dict(min_peaks=1, min_mz_range=0.0, scaling=None)


def _merge():
    rng = np.random.default_rng(51)
    mz = np.sort(rng.uniform(5, 2100, 3000)).astype(F32)
    it = rng.lognormal(0, 1.5, 3000).astype(F32)
    inr = (mz.astype(np.float64) >= 11) & (mz.astype(np.float64) <= 2010)
    for res in (-3, -2, -1, 0, 2):
        # groups of equal rounded m/z, summed in double
        r = np.round(mz[inr].astype(np.float64), res).astype(F32)
        uniq, inv = np.unique(r, return_inverse=True)
        sums = np.zeros(len(uniq))
        np.add.at(sums, inv, it[inr].astype(np.float64))
        thr = 0.01 * sums.max()
        lo, hi = int((sums > 1.01 * thr).sum()), int((sums > 0.99 * thr).sum())
        cnt = min(50, lo) if min(50, lo) == min(50, hi) else None   # known unless a sum sits on the threshold
        if res == -3:                                       # 0, 1000, 2000: runs of ~500 / ~1000 / ~500
            assert cnt == 3 and np.bincount(inv).max() > 900
        _add(f'merge_3000_res{res}', mz, it, dict(MERGE, resolution=res), True, count=cnt,
             out_mz=uniq if lo == hi == len(uniq) <= 50 else None, seed=res + 5)
    # one run spanning 10 orders of magnitude: the sequential fp32 sum shows in the last bit
    run = np.linspace(499.6, 500.4, 24)
    mz = np.sort(np.concatenate([_grid(30), run])).astype(F32)
    it = _flat(rng, len(mz))
    a = int(np.searchsorted(mz, F32(499.6)))
    mags = 10.0 ** rng.uniform(-5, 5, 24)
    mags[[2, 21]] = 1e5, 1e-5
    it[a:a + 24] = mags
    assert len(np.unique(np.round(mz.astype(np.float64)))) == 31
    _add('merge_magnitudes', mz, it, dict(MERGE, resolution=0, min_intensity=0.0), True, count=31)
    # exact .5 ties of the rounding go to even: 100.5 -> 100, 101.5 -> 102
    mz = np.concatenate([[100.0, 100.5, 101.5, 102.0], _grid(20, 200.0, 1900.0)])
    it = _flat(rng, 24)
    it[1], it[2] = 3.0, 3.0                                 # the .5 peaks carry the annotations
    _add('merge_half_even_res0', mz, it, dict(MERGE, resolution=0), True,
         src=np.concatenate([[1, 2], np.arange(4, 24)]),
         out_mz=np.concatenate([[100.0, 102.0], np.round(_grid(20, 200.0, 1900.0).astype(np.float64))]))
    # 250.125 * 100 = 25012.5 -> 25012, 250.375 * 100 = 25037.5 -> 25038 (both exact in fp32 and double)
    mz = np.array([250.12, 250.125, 250.375, 250.38, 600.0, 900.0], F32)
    it = np.array([1.0, 3.0, 3.0, 1.0, 2.0, 2.5], F32)
    _add('merge_half_even_res2', mz, it, dict(MERGE, resolution=2), True, src=[1, 2, 4, 5],
         out_mz=[250.12, 250.38, 600.0, 900.0])
    # the most intense peak of a run is tied: the FIRST one wins the annotation (np.argmax)
    mz = np.sort(np.concatenate([_grid(20), [499.8, 500.0, 500.2]])).astype(F32)
    it = _flat(rng, 23)
    a = int(np.searchsorted(mz, F32(499.8)))
    it[a:a + 3] = 5.0, 5.0, 1.0
    _add('merge_tied_best', mz, it, dict(MERGE, resolution=0), True,
         src=np.delete(np.arange(23), [a + 1, a + 2]))
    # in range before the rounding, on the window's bounds after it: they stay
    mz = np.concatenate([[11.4], _grid(20), [2009.6]])
    _add('merge_window_bounds', mz, _flat(rng, 22), dict(MERGE, resolution=0), True,
         src=np.arange(22), out_mz=np.concatenate([[11.0], np.round(_grid(20).astype(np.float64)), [2010.0]]))


# ---------------------------------------------------------------------------- 6. precursor removal
def _removal_masses(pmz, pz):
    neutral = (pmz - ADDUCT) * float(pz)                    # the oracle's expression, in double
    return [(neutral + iso) / c + ADDUCT for c in range(pz, 0, -1) for iso in range(3)]


def _precursor():
    rng = np.random.default_rng(61)
    # fewer than max_peaks peaks of similar intensity: everything that is not removed survives
    for pz, pmz in ((0, 500.0), (1, 500.0), (8, 300.0)):
        rm = [m for m in _removal_masses(pmz, pz) if 11 < m < 2010]
        assert len(rm) == {0: 0, 1: 3, 8: 21}[pz]
        planted = [500.0, 501.0, 502.0] if pz == 0 else rm   # z = 0: the loop does not run, they stay
        mz = np.sort(np.concatenate([_grid(26), planted]).astype(F32))
        hit = np.array([any(abs(float(m) - r) <= 0.05 for r in _removal_masses(pmz, pz)) for m in mz],
                       bool)
        assert hit.sum() == len(rm) and len(mz) - hit.sum() <= 50
        _add(f'precursor_z{pz}', mz, _flat(rng, len(mz)), dict(remove_precursor=True, rp_tol=0.05),
             True, src=np.nonzero(~hit)[0], pmz=pmz, pz=pz, seed=pz)
    # inclusive '<= tolerance': d is the peak's distance to its nearest removal mass, in double
    pmz, pz = 500.3, 3
    mz = np.sort(np.concatenate([_grid(40), [500.1]])).astype(F32)
    a = int(np.searchsorted(mz, F32(500.1)))
    dist = np.array([[abs(float(m) - r) for r in _removal_masses(pmz, pz)] for m in mz])
    d = float(dist[a].min())
    assert 0.1 < d < 0.3 and np.delete(dist.min(1), a).min() > 2 * d
    it = _flat(rng, 41)
    _add('precursor_tol_equal', mz, it, dict(remove_precursor=True, rp_tol=d), True,
         src=np.delete(np.arange(41), a), pmz=pmz, pz=pz)
    _add('precursor_tol_below', mz, it, dict(remove_precursor=True, rp_tol=float(np.nextafter(d, 0.0))),
         True, src=np.arange(41), pmz=pmz, pz=pz)


# ---------------------------------------------------------------------------- 7. bad intensities
def _bad():
    rng = np.random.default_rng(71)
    base = _flat(rng, 40)

    def one(name, v, valid):
        it = base.copy()
        it[13] = v
        _add(name, _grid(40), it, dict(), valid, src=np.delete(np.arange(40), 13) if valid else None)
    one('bad_one_zero', 0.0, True)
    one('bad_one_negative_zero', -0.0, True)
    one('bad_one_negative', -1.5, True)
    one('bad_one_inf', np.inf, False)                       # nothing is above an infinite threshold
    one('bad_one_nan_pos', NAN_POS, False)                  # intensity.max() is NaN: nothing is above it
    one('bad_one_nan_neg', NAN_NEG, False)
    assert np.signbit(CASES[-1].intensity[13]) and not np.signbit(CASES[-2].intensity[13])
    _add('bad_all_zero', _grid(40), np.zeros(40), dict(), False)
    _add('bad_all_nan', _grid(40), np.full(40, NAN_NEG), dict(), False)
    # a NaN that never reaches the intensity filter changes nothing
    mz = np.concatenate([[5.0], _grid(40)])
    _add('bad_nan_out_of_range', mz, np.concatenate([[NAN_NEG], base]), dict(), True,
         src=np.arange(1, 41))
    mz = np.sort(np.concatenate([_grid(40), [500.0]])).astype(F32)
    a = int(np.searchsorted(mz, F32(500.0)))
    _add('bad_nan_on_precursor', mz, np.insert(base, a, NAN_POS),
         dict(remove_precursor=True, rp_tol=0.1), True, src=np.delete(np.arange(41), a),
         pmz=500.0, pz=1)
    # a NaN inside a merged run poisons the run's sum
    mz = np.sort(np.concatenate([_grid(40), [499.9, 500.1]])).astype(F32)
    it = _flat(rng, 42)
    it[int(np.searchsorted(mz, F32(500.1)))] = NAN_NEG
    _add('bad_nan_merged', mz, it, dict(resolution=0), False)


_sort_sizes()
_ties()
_threshold()
_validity()
_merge()
_precursor()
_bad()
