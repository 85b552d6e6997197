"""Rescoring cases on the numeric boundaries of the two fast kernels (csrc/rescore.hip): spectra
whose candidate peaks sit on the edge of a query peak's window ``|qm - (cm + pmd / s)| = tol``, in
every regime of fragment m/z, precursor mass difference and tolerance that the fp32 bin filter of
``rescore_flat_kernel`` / ``score_two`` has to survive or has to hand to the binary-search kernel.
Plain numpy, no GPU: ``tests/test_rescore_cases_cpu.py`` counts (with the oracle) what was planted,
``tests/test_gpu_rescore_numeric.py`` runs it through the kernels.

A regime is a list of BLOCKS; a block is one call's worth of spectra at one tolerance: queries of
1, 37 and 100 peaks, and for every query one candidate per (precursor charge z, target pmd) of the
block. ``Block.owner[r]`` is the query that library row r was planted for.

Candidate peak j picks a distinct query peak i, a shift s in 0 .. z, a side and a k in 4 .. 20,
and is placed at ``float32(qm_i +- tol * (1 - 2^-k) - pmd / s)``, then moved by -2 .. +2 float32
ulps: some land just inside the window, some on its edge, some just outside. Half of them carry
the fragment charge s, half carry 0 (product factor 2/3). About one candidate in five gets a twin
peak inside the same query window (a doubly matched peak: the flat kernel hands the candidate to the
pair kernel)."""
from dataclasses import dataclass

import numpy as np

QN = (1, 37, 100)          # query peaks: one lane, part of a wave, the hash path's limit (RS_HQ_MAX)
CN_MAX = 64                # candidate peaks the fast kernels take
K_RANGE = (4, 21)          # distance from the window edge: tol * 2^-k
Z_FLAT = (1, 2, 3, 4)      # precursor charges the flat kernel's shift table holds
Z_PAIR = (5, 8, 30)        # ... and the ones it leaves to the pair kernel

# The bin filter's accepted envelope (csrc/rescore.hip, DESIGN.md "Rescoring: numeric envelope"):
# candidates with |pmd| above RS_MD_ENV leave the fast kernels, and a query is hashed only while
# margin(tol, largest query m/z) <= 0.45 bins.
RS_MD_ENV = 4096.0
RS_MARGIN_MAX = 0.45


def margin(tol, q_abs_max):
    """The filter margin of a query, in bins (the expression of the kernels)."""
    return 1e-3 + (0.5 / tol) * 6.0e-8 * (RS_MD_ENV + 3.0 * (q_abs_max + tol))


def threshold_tol(q_abs_max):
    """Smallest tolerance at which a query whose largest m/z is q_abs_max is still hashed."""
    lo, hi = 1e-6, 1.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if margin(mid, q_abs_max) <= RS_MARGIN_MAX else (mid, hi)
    return hi


@dataclass
class Block:
    name: str
    tol: float
    queries: tuple          # (offsets, mz, intensity, charge, precursor_mz, precursor_charge)
    library: tuple
    owner: np.ndarray       # [library rows] query index

    def packed(self):
        from ann_solo_amd.packed import PackedSpectra
        return PackedSpectra.from_numpy(*self.queries), PackedSpectra.from_numpy(*self.library)

    @property
    def nq(self):
        return len(self.queries[0]) - 1

    @property
    def nlib(self):
        return len(self.library[0]) - 1


def _nudge(x32, n):
    """x32 (positive float32) moved by n float32 ulps."""
    return (np.asarray(x32, np.float32).view(np.int32) + np.asarray(n, np.int32)).view(np.float32)


def _query_mz(rng, qn, lo, hi, tol):
    """qn ascending float32 m/z in [lo, hi], at least 8 * tol apart (after the float32 rounding)."""
    gap = 8.0 * tol + 2.0 * float(np.spacing(np.float32(hi)))
    room = (hi - lo) - gap * (qn - 1)
    assert room > 0, (qn, lo, hi, tol)
    mz = (lo + np.sort(rng.uniform(0, room, qn)) + gap * np.arange(qn)).astype(np.float32)
    assert np.all(np.diff(mz.astype(np.float64)) >= 8.0 * tol) and mz[0] > 0
    return mz


def _intensity(rng, n):
    it = rng.lognormal(0, 1, n).astype(np.float32)
    return (it / np.float32(max(np.linalg.norm(it), 1e-30))).astype(np.float32)


def _candidate(rng, qmz, tol, pmd, z):
    """One candidate spectrum planted on the windows of the query peaks qmz."""
    qn = len(qmz)
    cn = min(qn, int(rng.integers(CN_MAX // 2, CN_MAX + 1)))
    twin = qn > 1 and rng.random() < 0.2
    picks = rng.choice(qn, cn - (1 if twin and cn == CN_MAX else 0), replace=False)
    if twin:
        picks = np.concatenate([picks, picks[:1]])
    n = len(picks)
    s = rng.integers(0, z + 1, n)
    if twin:
        s[-1] = s[0]                       # the twin sits in the same window at the same shift
    side = rng.choice([-1.0, 1.0], n)
    k = rng.integers(K_RANGE[0], K_RANGE[1], n)
    md = np.where(s > 0, pmd / np.maximum(s, 1), 0.0)
    pos = qmz[picks].astype(np.float64) + side * tol * (1.0 - 2.0 ** -k.astype(np.float64)) - md
    # a peak has a positive m/z: where the shift would put it below zero it is planted unshifted
    bad = pos <= 1e-6
    s[bad] = 0
    pos[bad] = (qmz[picks].astype(np.float64) + side * tol * (1.0 - 2.0 ** -k.astype(np.float64)))[bad]
    pos = np.maximum(pos, 1e-6)
    mz = _nudge(pos.astype(np.float32), rng.integers(-2, 3, n))
    chg = np.where(rng.random(n) < 0.5, s, 0)
    chg = np.where(s == 0, rng.integers(0, min(z, 255) + 1, n), chg).astype(np.uint8)
    order = np.argsort(mz, kind='stable')
    return mz[order], _intensity(rng, n)[order], chg[order]


def pack(spectra, pmz, pz):
    """Spectra [(mz, intensity, charge), ...] with their precursors as the six packed arrays."""
    offs = np.concatenate([[0], np.cumsum([len(s[0]) for s in spectra])]).astype(np.int64)
    cat = lambda i, dt: np.concatenate([s[i] for s in spectra]).astype(dt)
    return (offs, cat(0, np.float32), cat(1, np.float32), cat(2, np.uint8),
            np.asarray(pmz, np.float64), np.asarray(pz, np.int64))


def make_block(name, seed, mz_range, tol, specs, reps, qns=QN):
    """specs: (z, pmd target) per candidate of a query (the target's sign is the sign of pmd);
    reps: queries per peak count."""
    rng = np.random.default_rng(seed)
    qs, q_pmz, ls, l_pmz, l_z, owner = [], [], [], [], [], []
    for qn in qns:
        for _ in range(reps):
            qmz = _query_mz(rng, qn, mz_range[0], mz_range[1], tol)
            qi = len(qs)
            qs.append((qmz, _intensity(rng, qn), np.zeros(qn, np.uint8)))
            # precursors: both positive, (q_pmz - c_pmz) * z on the target. One query precursor
            # serves all of its candidates, so it carries the largest offset of the block.
            far = max([abs(t) / z for z, t in specs if t > 0], default=0.0)
            qp = float(rng.uniform(400, 900)) + far
            q_pmz.append(qp)
            for z, target in specs:
                cp = qp - target / z
                assert cp > 0
                pmd = (qp - cp) * float(z)            # as the kernels and the reference compute it
                ls.append(_candidate(rng, qmz, tol, pmd, z))
                l_pmz.append(cp)
                l_z.append(z)
                owner.append(qi)
    return Block(name, tol, pack(qs, q_pmz, np.full(len(qs), 2)), pack(ls, l_pmz, l_z),
                 np.asarray(owner, np.int64))


def _specs(rng, zs, pmd_abs, signs=(-1.0, 1.0)):
    """One candidate per (z, sign); |pmd| drawn from pmd_abs = (lo, hi) or fixed when a number."""
    out = []
    for z in zs:
        for sg in signs:
            a = float(rng.uniform(*pmd_abs)) if isinstance(pmd_abs, tuple) else float(pmd_abs)
            out.append((z, sg * a))
    return out


def regime(number):
    """The blocks of regime 1 .. 5 (deterministic)."""
    rng = np.random.default_rng(1000 + number)
    blocks = []

    def add(tag, mz_range, tol, specs, reps, qns=QN):
        blocks.append(make_block(f'r{number}:{tag}:mz{mz_range[0]:g}-{mz_range[1]:g}:tol{tol:g}',
                                 10_000 * number + len(blocks), mz_range, tol, specs, reps, qns))

    if number == 1:        # inside the envelope, and |pmd| right up to its edge on both sides of it
        for mzr in ((100.0, 2000.0), (2000.0, 2600.0)):
            # ... and the smallest tolerance at which every query of the m/z range is still hashed
            for tol in (0.02, 0.05, 0.001, threshold_tol(mzr[1]) * 1.001):
                specs = _specs(rng, Z_FLAT + Z_PAIR, (1.0, 2000.0)) + \
                    [(2, -(RS_MD_ENV - 0.01)), (3, RS_MD_ENV - 0.01), (4, -(RS_MD_ENV + 0.01)),
                     (8, -(RS_MD_ENV - 0.01)), (30, -(RS_MD_ENV + 0.01))]
                add('in', mzr, tol, specs, 1)
    elif number == 2:      # low end: windows that reach below zero, negative shifts and bins
        for tol in (0.001, 0.005):
            add('low', (0.001, 5.0), tol, _specs(rng, Z_FLAT + (5, 8), (1.0, 2000.0), (-1.0,)), 10)
    elif number == 3:      # the tolerance at which a query leaves the hash path
        mzr = (2000.0, 2600.0)
        t = threshold_tol(2600.0)
        for tol in (0.00076, 0.00077, t * 0.98, t * 1.02):
            add('route', mzr, tol, _specs(rng, Z_FLAT + (5, 8), (1.0, 2000.0)), 3)
    elif number == 4:      # beyond the old envelope by fragment m/z
        for mzr, reps in (((2600.0, 5000.0), 1), ((5000.0, 20000.0), 1), ((20000.0, 100000.0), 3)):
            for tol in (0.02, 0.001):
                # where ulp(m/z) exceeds the tolerance few planted peaks land inside a window
                more = 4 if (tol < 0.01 and mzr[0] >= 5000.0) else 1
                add('mz', mzr, tol, _specs(rng, Z_FLAT + Z_PAIR, (1.0, 2000.0)), reps * more)
    elif number == 5:      # beyond it by precursor mass difference: far precursor, high charge
        # (only the NEGATIVE targets put far-shifted peaks to the test: with pmd = +2e4 / +1e5 the
        # shifted position qm - pmd / s lies below zero for every s <= 30, so those candidates'
        # peaks are planted unshifted and their far shifts merely have to match nothing)
        for tol in (0.02, 0.001):
            for a in (2e4, 1e5):
                add(f'pmd{a:g}', (100.0, 2600.0), tol, _specs(rng, (4, 30), a) + _specs(rng, (4, 30), a), 4)
    else:
        raise ValueError(number)
    return blocks


REGIMES = (1, 2, 3, 4, 5)
_CACHE = {}


def regime_blocks(number):
    """``regime(number)``, built once per process and shared (callers must not modify it)."""
    if number not in _CACHE:
        _CACHE[number] = regime(number)
    return _CACHE[number]


def grouped_lists(block, length=40):
    """Candidate lists of `length` per query: the rows planted for the query first (a query has
    fewer than `length`), then rows planted for the other queries of the block. CSR (rows, offsets)."""
    rows, off = [], [0]
    for q in range(block.nq):
        own = np.nonzero(block.owner == q)[0]
        other = np.nonzero(block.owner != q)[0]
        take = np.concatenate([own, np.roll(other, -7 * q)])[:length]
        rows.append(np.sort(take))
        off.append(off[-1] + len(take))
    return np.concatenate(rows).astype(np.int64), np.asarray(off, np.int32)


def boundary_stats(O, block):
    """(matched peaks, matched peaks within 4 float32 ulps of the window edge at a shift they
    take part in and match at) over the block's planted pairs, from the oracle's greedy matches."""
    qo, qmz, qit, _, qpmz, _ = block.queries
    lo, lmz, lit, lch, lpmz, lz = block.library
    n_match = n_edge = 0
    for r in range(block.nlib):
        q = int(block.owner[r])
        a, b = slice(qo[q], qo[q + 1]), slice(lo[r], lo[r + 1])
        _, m = O.dot_pair(qmz[a], qit[a], qpmz[q], lmz[b], lit[b], lch[b], lpmz[r], int(lz[r]),
                          block.tol, True)
        if not len(m):
            continue
        qm = qmz[a][m[:, 0]].astype(np.float64)
        cm32 = lmz[b][m[:, 1]]
        cm = cm32.astype(np.float64)
        pmd = (qpmz[q] - lpmz[r]) * float(lz[r])
        md = np.concatenate([[0.0], pmd / np.arange(1, int(lz[r]) + 1)])       # every shift
        dist = np.abs(qm[:, None] - (cm[:, None] + md[None, :]))
        ulp = np.spacing(np.maximum(cm32, qmz[a][m[:, 0]])).astype(np.float64)
        # only the shifts the peak takes part in: every one for an unannotated peak, else 0 and
        # its fragment charge -- and only where it matches there
        cc = lch[b][m[:, 1]].astype(np.int64)[:, None]
        sh = np.arange(len(md))[None, :]
        can = (cc == 0) | (sh == 0) | (sh == cc)
        near = can & (np.abs(dist - block.tol) <= 4.0 * ulp[:, None]) & (dist <= block.tol)
        n_match += len(m)
        n_edge += int(near.any(axis=1).sum())
    return n_match, n_edge


# ------------------------------------------------------------------ exact-sum gate
GATE_E = 120                       # exponent byte of the big products
GATE_D = (22, 23, 24, 25, 40)      # exponent spread: <= 23 the unordered sum is exact, beyond it is not
# (small products, where): the issue's single odd-mantissa product, and several of them -- ONE small
# term sees one rounding in any order; two or more add exactly among themselves while the partial
# sum is small (they arrive first) but lose their last bits one by one behind the big products
# (sorted order), so only these tell an off-by-one gate from the right one
GATE_SMALL = ((1, 'random'), (2, 'first'), (8, 'first'), (8, 'random'), (8, 'last'))
GATE_SHAPES = ((64, 2), (32, 2), (64, 5), (32, 5), (64, 31))     # (candidate peaks, precursor charge)


def _f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def gate_case(shifted):
    """Queries of 64 and 100 peaks with q_int = 1.0; candidates whose peaks sit exactly on 64 (or 32)
    of the query's m/z (shifted: 3 Da below, fragment charge 0, so the product is
    (float)(2/3 * c_int)): intensities with an all-ones mantissa at exponent E, and k with an odd
    mantissa at exponent E - d on the first, the last or random peaks. Returns (queries, library,
    owner, meta) with meta[r] = (candidate peaks, z, d, k, where)."""
    mz100 = (200.0 + 10.0 * np.arange(100)).astype(np.float32)
    queries = [(mz100[:64], np.ones(64, np.float32), np.zeros(64, np.uint8)),
               (mz100, np.ones(100, np.float32), np.zeros(100, np.uint8))]
    q_pmz = [501.5 if shifted else 500.0] * 2
    lib, owner, l_z, meta = [], [], [], []
    rng = np.random.default_rng(3)
    for qi, qn in ((0, 64), (1, 100)):
        for cn, z in GATE_SHAPES:
            for d in GATE_D:
                for k, where in GATE_SMALL:
                    at = np.sort(rng.choice(qn, cn, replace=False))
                    inten = _f32(np.full(cn, (GATE_E << 23) | 0x7FFFFF, np.uint32)).copy()
                    pos = (np.arange(k) if where == 'first' else np.arange(cn - k, cn) if where == 'last'
                           else rng.choice(cn, k, replace=False))
                    mant = np.array([1], np.uint32) if k == 1 else (rng.integers(0, 1 << 22, k).astype(np.uint32) << 1) | 1
                    inten[pos] = _f32(np.uint32((GATE_E - d) << 23) | mant)
                    mz = mz100[at] - np.float32(3.0 if shifted else 0.0)
                    lib.append((mz.astype(np.float32), inten, np.zeros(cn, np.uint8)))
                    owner.append(qi)
                    l_z.append(z)
                    meta.append((cn, z, d, k, where))
    # pmd = (q_pmz - c_pmz) * z = 3 exactly for every z (shifted), else 0: no shift at all
    l_pmz = [501.5 - 3.0 / z if shifted else 500.0 for z in l_z]
    return pack(queries, q_pmz, [2, 2]), pack(lib, l_pmz, l_z), np.asarray(owner), meta


def gate_products(library, r, shifted):
    """The fp32 products of library row r of a gate case, in candidate-peak (m/z) order: every
    peak matches one query peak of intensity 1.0, with factor 1 or (shifted, charge 0) 2/3."""
    o = library[0]
    c = library[2][o[r]:o[r + 1]].astype(np.float64)
    return ((2.0 / 3.0) * 1.0 * c if shifted else c).astype(np.float32)


def sum_in_order(products):
    s = 0.0
    for v in np.asarray(products, np.float64).tolist():
        s += v
    return s
