"""Rescoring cases for the ppm fragment tolerance (include/annsolo_mi.h: ASL_SCORE_FRAGMENT_PPM), in
the style of tests/rescore_cases.py: spectra whose candidate peaks sit on the edge of a query peak's
window -- a window whose width now depends on the QUERY peak, tol_i = ppm * 1e-6 * qm_i.
Plain numpy, no GPU: tests/test_ppm_cpu.py counts (with tests/ppm_ref.py) what was planted,
tests/test_gpu_ppm.py runs it through the kernels.

A block is one call's worth of spectra at one tolerance:

* queries of 1, 37, 100 and 101 peaks over m/z 100 .. 2000 (101: beyond the hash path's limit, the
  whole query goes to the binary-search kernel), at least 8 tol_i(2000) apart;
* for every query one candidate of <= 64 peaks per (precursor charge z in 1 .. 4, 5, 8; sign of pmd),
  two of 65 .. 80 peaks (the fast kernels take <= 64: binary-search kernel), and one GATE candidate
  whose |pmd| lies within an ulp of the shift gate's threshold rel * q_pmz (ppm_ref.shift_gate);
* candidate peak j picks a query peak i, a shift s in 0 .. z, a side and a k in 4 .. 20 and is placed
  at float32(qm_i +- tol_i (1 - 2^-k) - pmd / s), then moved by -2 .. +2 float32 ulps;
* about one candidate in five gets a twin peak inside the same query window (a doubly matched peak).

``Block.owner[r]`` is the query library row r was planted for; ``Block.gate[r]`` is +1 / -1 for a gate
candidate whose |pmd| is >= / < the threshold (0: an ordinary candidate)."""
from dataclasses import dataclass

import numpy as np

import ppm_ref as PR
import rescore_cases as RC

QN = (1, 37, 100, 101)
MZ_RANGE = (100.0, 2000.0)
Z_ALL = (1, 2, 3, 4, 5, 8)
PPM = (5.0, 10.0, 20.0, 50.0)
# tol_max = 0.2e-6 * 2000 = 4e-4 lies below the smallest width the bin filter still hashes at m/z 2000
# (RC.threshold_tol(2000) = 6.8e-4): every query of this block is deferred whole
PPM_DEFERRED = 0.2
BIG = (65, 81)             # peaks of the candidates beyond the fast kernels


@dataclass
class Block:
    name: str
    ppm: float
    queries: tuple          # (offsets, mz, intensity, charge, precursor_mz, precursor_charge)
    library: tuple
    owner: np.ndarray       # [library rows] query index
    gate: np.ndarray        # [library rows] +1 / -1: gate candidate at / below the threshold; 0: ordinary

    def packed(self):
        from ann_solo_amd.packed import PackedSpectra
        return PackedSpectra.from_numpy(*self.queries), PackedSpectra.from_numpy(*self.library)

    @property
    def nq(self):
        return len(self.queries[0]) - 1

    @property
    def nlib(self):
        return len(self.library[0]) - 1


def _candidate(rng, qmz, ppm, pmd, z, cn=None):
    """One candidate planted on the ppm windows of the query peaks qmz (RC._candidate with tol_i)."""
    qn = len(qmz)
    big = cn is not None
    if not big:
        cn = min(qn, int(rng.integers(RC.CN_MAX // 2, RC.CN_MAX + 1)))
    twin = not big and qn > 1 and rng.random() < 0.2
    # (a big candidate of a short query plants several peaks per window)
    picks = rng.choice(qn, cn - (1 if twin and cn == RC.CN_MAX else 0), replace=big and qn < cn)
    if twin:
        picks = np.concatenate([picks, picks[:1]])
    n = len(picks)
    s = rng.integers(0, z + 1, n)
    if twin:
        s[-1] = s[0]
    side = rng.choice([-1.0, 1.0], n)
    k = rng.integers(RC.K_RANGE[0], RC.K_RANGE[1], n)
    md = np.where(s > 0, pmd / np.maximum(s, 1), 0.0)
    tl = PR.peak_tol(qmz, ppm, 'ppm')[picks]
    edge = qmz[picks].astype(np.float64) + side * tl * (1.0 - 2.0 ** -k.astype(np.float64))
    pos = edge - md
    bad = pos <= 1.0           # a peak has a positive m/z: planted unshifted where the shift would not
    s[bad] = 0
    pos[bad] = edge[bad]
    mz = RC._nudge(pos.astype(np.float32), rng.integers(-2, 3, n))
    chg = np.where(rng.random(n) < 0.5, s, 0)
    chg = np.where(s == 0, rng.integers(0, z + 1, n), chg).astype(np.uint8)
    order = np.argsort(mz, kind='stable')
    return mz[order], RC._intensity(rng, n)[order], chg[order]


def _gate_precursors(rng, ppm, z, above, sign):
    """(q_pmz, c_pmz): pmd = (q_pmz - c_pmz) * z is exact and |pmd| lies within one ulp of the gate's
    threshold g = rel * q_pmz -- |pmd| >= g (`above`: the shifts are on by the narrowest margin) or
    |pmd| < g. Both precursors lie on the fp64 grid of [512, 1024), so their difference is exact; the
    search walks that grid until the threshold's own rounding falls on the wanted side."""
    rel = PR.rel_tol(ppm)
    grid = 2.0 ** -43
    for _ in range(10000):
        q0 = float(rng.uniform(560.0, 980.0))
        d = round(float(rel * q0) / z / grid) * grid          # the precursors' distance, on the grid
        pmd = np.float64(d) * np.float64(z)
        assert float(pmd) / z == d                              # exact
        qc = round(float(pmd / rel) / grid) * grid
        for t in range(-4, 5):
            q = qc + t * grid
            g = rel * np.float64(q)
            ulps = (float(pmd) - float(g)) / float(np.spacing(g))
            if (0.0 <= ulps <= 1.0) if above else (-1.0 <= ulps < 0.0):
                c = q - sign * d
                got = (np.float64(q) - np.float64(c)) * np.float64(z)
                assert abs(got) == pmd and (abs(got) >= g) == above
                return q, c
    raise AssertionError('no precursor pair on the gate')


def make_block(name, seed, ppm, reps, qns=QN):
    rng = np.random.default_rng(seed)
    tol_max = float(PR.rel_tol(ppm)) * MZ_RANGE[1]
    qs, q_pmz, ls, l_pmz, l_z, owner, gate = [], [], [], [], [], [], []
    for qn in qns:
        for rep in range(reps):
            qmz = RC._query_mz(rng, qn, MZ_RANGE[0], MZ_RANGE[1], tol_max)
            qi = len(qs)
            qs.append((qmz, RC._intensity(rng, qn), np.zeros(qn, np.uint8)))
            # the gate candidate fixes the query's precursor; the other candidates follow it
            gz = int(rng.choice([2, 3, 4]))
            above = bool((qi + rep + qn) % 2)
            qp, gc = _gate_precursors(rng, ppm, gz, above, float(rng.choice([-1.0, 1.0])))
            q_pmz.append(qp)
            specs = [(z, sg * float(rng.uniform(1.0, 500.0)), None) for z in Z_ALL for sg in (-1.0, 1.0)]
            specs += [(z, -float(rng.uniform(1.0, 500.0)), int(rng.integers(*BIG))) for z in (2, 5)]
            for z, target, cn in specs:
                cp = qp - target / z
                assert cp > 0
                pmd = (qp - cp) * float(z)
                ls.append(_candidate(rng, qmz, ppm, pmd, z, cn))
                l_pmz.append(cp)
                l_z.append(z)
                owner.append(qi)
                gate.append(0)
            ls.append(_candidate(rng, qmz, ppm, (qp - gc) * float(gz), gz))
            l_pmz.append(gc)
            l_z.append(gz)
            owner.append(qi)
            gate.append(1 if above else -1)
    return Block(name, ppm, RC.pack(qs, q_pmz, np.full(len(qs), 2)), RC.pack(ls, l_pmz, l_z),
                 np.asarray(owner, np.int64), np.asarray(gate, np.int64))


_CACHE = {}


def blocks():
    """The blocks (deterministic), built once per process and shared: callers must not modify them.
    16 queries and 240 library spectra each."""
    if not _CACHE:
        out = [make_block(f'ppm{p:g}', 77_000 + i, p, 4) for i, p in enumerate(PPM)]
        out.append(make_block(f'ppm{PPM_DEFERRED:g}:deferred', 77_100, PPM_DEFERRED, 4))
        _CACHE['blocks'] = out
    return _CACHE['blocks']


def grouped_lists(block, length=40):
    return RC.grouped_lists(block, length)


def window_stats(block):
    """Over the block's planted pairs and the shifts a candidate peak takes part in: how many
    (query peak, candidate peak, shift) lie within 4 float32 ulps of the window's edge INSIDE it
    (dist <= tol_i), how many OUTSIDE (dist > tol_i), and how many are ON it -- the planted float32 is
    the one nearest to the exact edge (| dist - tol_i | <= half a float32 ulp). In the restatement's
    arithmetic."""
    qo, qmz, _, _, qpmz, _ = block.queries
    lo, lmz, _, lch, lpmz, lz = block.library
    inside = outside = on = 0
    for r in range(block.nlib):
        q = int(block.owner[r])
        qm32 = qmz[qo[q]:qo[q + 1]]
        cm32 = lmz[lo[r]:lo[r + 1]]
        qm, cm = qm32.astype(np.float64), cm32.astype(np.float64)
        tl = PR.peak_tol(qm32, block.ppm, 'ppm')
        S, pmd = PR.num_shifts(qpmz[q], lpmz[r], int(lz[r]), block.ppm, True, 'ppm')
        cc = lch[lo[r]:lo[r + 1]].astype(np.int64)
        ulp = np.spacing(np.maximum(qm32[:, None], cm32[None, :])).astype(np.float64)
        for s in range(S):
            md = 0.0 if s == 0 else pmd / np.float64(s)
            dist = np.abs(qm[:, None] - (cm[None, :] + md))
            can = ((cc == 0) | (cc == s) | (s == 0))[None, :]
            near = can & (np.abs(dist - tl[:, None]) <= 4.0 * ulp)
            inside += int((near & (dist <= tl[:, None])).sum())
            outside += int((near & (dist > tl[:, None])).sum())
            on += int((can & (np.abs(dist - tl[:, None]) <= 0.5 * ulp)).sum())
    return inside, outside, on
