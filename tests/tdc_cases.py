"""Seeded inputs of ``asl_tdc_qvalues`` shared by test_tdc_cpu.py and test_gpu_tdc.py: every builder returns
``(score, is_target, group, use, desc)`` (``group`` / ``use`` may be ``None``).

Sizes: 0, 1, 2; 63 .. 65 (a wave); 255 .. 257 (a workgroup, and a block of every scan level); TILE - 1 .. TILE + 1
(the sort's tile, ``ASL_TDC_TILE`` read from the header); and two large ones,

  * ``N_LEVELS`` = 257 * TILE + 1 = 263 169: 258 sort tiles, so the digit counts of a pass are 256 * 258 elements,
    their scan has 258 block partials -- more than one block of 256 -- and the scan of the partials itself needs
    a second level; the row scans (counts, q) run 1 029 blocks and three levels; every kernel runs several
    workgroups, the last tile holds a single key;
  * 300 001, the size of a large training part, which takes the same paths with a ragged last tile.
"""
import contextlib
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, '..', 'include', 'annsolo_mi.h')) as _f:
    TILE = int(re.search(r'#define\s+ASL_TDC_TILE\s+(\d+)', _f.read()).group(1))

SMALL_SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1)
N_LEVELS = 257 * TILE + 1
LARGE_SIZES = (N_LEVELS, 300001)
SCORES = ('equal', 'distinct', 'eight', 'zeros', 'signed', 'denormal', 'inf', 'lowbyte', 'highbyte')
TARGETS = ('all', 'none', 'best_decoys', 'half', 'most')
GROUPS = ('null', 'one', 'mixed', 'extremes', 'singles')
USES = ('null', 'zero', 'half', 'one')


def scores(kind: str, n: int, rng) -> np.ndarray:
    if kind == 'equal':                 # one run
        return np.full(n, 0.625)
    if kind == 'distinct':
        return rng.permutation(n).astype(np.float64) / max(n, 1)
    if kind == 'eight':                 # long runs
        return rng.integers(0, 8, n) / 8.0
    if kind == 'zeros':                 # -0.0 and +0.0 are one run, with neighbours on both sides
        return rng.choice(np.array([-1e-300, -5e-324, -0.0, 0.0, 5e-324, 1e-300]), n)
    if kind == 'signed':
        return rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, n)
    if kind == 'denormal':              # +-k * 2^-1074 from the bit patterns: no arithmetic that could flush them
        k = rng.integers(-40, 41, n)
        return (np.abs(k).astype(np.uint64) | ((k < 0).astype(np.uint64) << np.uint64(63))).view(np.float64)
    if kind == 'inf':
        return rng.choice(np.array([-np.inf, -1.0, 0.5, 2.0, np.inf]), n)
    if kind == 'lowbyte':               # only the lowest byte of the bit pattern differs: one radix pass matters
        bits = np.float64(0.7).view(np.uint64) & ~np.uint64(0xff)
        return (bits | rng.integers(0, 256, n).astype(np.uint64)).view(np.float64)
    if kind == 'highbyte':              # only the highest byte differs (the byte below is 0: never inf or NaN)
        return ((rng.integers(0, 256, n).astype(np.uint64) << np.uint64(56))
                | np.uint64(0x0000123456789abc)).view(np.float64)
    raise ValueError(kind)


def targets(kind: str, score, desc: bool, rng) -> np.ndarray:
    n = len(score)
    if kind == 'all':
        return np.ones(n, bool)
    if kind == 'none':
        return np.zeros(n, bool)
    if kind == 'best_decoys':           # the best third are decoys: FDR 1 while there is no target yet
        t = rng.random(n) < 0.7
        order = np.argsort(-score if desc else score, kind='stable')
        t[order[:(n + 2) // 3]] = False
        return t
    return rng.random(n) < (0.5 if kind == 'half' else 0.95)


def groups(kind: str, n: int, rng):
    if kind == 'null':
        return None
    if kind == 'one':
        return np.full(n, 7, np.int32)
    if kind == 'mixed':                 # ids -1 .. 5 of unequal sizes; id 4 has one row, id 5 two (where n allows)
        g = rng.choice(np.arange(-1, 4), n, p=[0.4, 0.3, 0.15, 0.1, 0.05]).astype(np.int32)
        spots = rng.permutation(n)[:3]
        g[spots[:1]] = 4
        g[spots[1:3]] = 5
        return g
    if kind == 'extremes':
        lim = np.iinfo(np.int32)
        return rng.choice(np.array([lim.min, -1, 0, lim.max], np.int32), n)
    if kind == 'singles':               # n groups of one row each
        return (rng.permutation(n) - n // 2).astype(np.int32)
    raise ValueError(kind)


def uses(kind: str, n: int, rng):
    if kind == 'null':
        return None
    u = np.zeros(n, np.uint8)
    if kind == 'half':
        u[rng.random(n) < 0.5] = 1
    elif kind == 'one' and n:
        u[int(rng.integers(n))] = 1
    return u


def build(n: int, score: str, target: str, group: str, use: str, desc: bool):
    rng = np.random.default_rng([n, SCORES.index(score), TARGETS.index(target), GROUPS.index(group),
                                 USES.index(use), int(desc)])
    s = scores(score, n, rng)
    return s, targets(target, s, desc, rng), groups(group, n, rng), uses(use, n, rng), desc


def case_ids():
    """``(id, arguments of build)``: every (small size, group) pair with the score kinds cycling so that every
    (score, group) pair occurs, targets and ``use`` cycling; a handful at the large sizes; all of it once per
    direction."""
    out = []
    for si, n in enumerate(SMALL_SIZES):
        for gi, group in enumerate(GROUPS):
            k = si * len(GROUPS) + gi
            out.append((n, SCORES[k % len(SCORES)], TARGETS[(si + gi) % len(TARGETS)], group,
                        USES[(k // 2) % len(USES)]))
    for n in LARGE_SIZES:
        out += [(n, 'distinct', 'half', 'null', 'null'), (n, 'eight', 'most', 'mixed', 'half'),
                (n, 'signed', 'best_decoys', 'extremes', 'null')]
    out += [(N_LEVELS, 'lowbyte', 'most', 'one', 'half'), (300001, 'highbyte', 'half', 'null', 'half')]
    return [('-'.join(map(str, c)) + ('-desc' if desc else '-asc'), c + (desc,)) for c in out
            for desc in (True, False)]


CASE_IDS = case_ids()
_built, _host_q = {}, {}


@contextlib.contextmanager
def ieee_denormals():
    """numpy as it is by default. A library loaded earlier in a test session may have left the thread flushing
    denormals to zero (FTZ / DAZ): numpy then compares 5e-324 equal to 0 and the host code no longer computes what
    it computes in a fresh interpreter -- the reference the device, which keeps fp64 denormals, is held to."""
    import torch
    tiny = np.array([1], np.uint64).view(np.float64)
    flushing = bool((tiny * 1.0).view(np.uint64)[0] == 0)
    if flushing:
        torch.set_flush_denormal(False)
    try:
        yield
    finally:
        if flushing:
            torch.set_flush_denormal(True)


def host_q(name: str) -> np.ndarray:
    """The reference of every comparison, computed once per case: ``fdr.tdc_qvalues`` per group
    (``fdr._grouped_q``; the same loop with ``desc`` handed on for the ascending direction) over the used rows,
    ``use`` applied by subsetting first; NaN for the unused rows."""
    from ann_solo_amd import fdr
    if name not in _host_q:
        score, target, group, use, desc = get(name)
        n = len(score)
        rows = np.arange(n) if use is None else np.nonzero(use)[0]
        s, t = score[rows], target[rows]
        g = np.zeros(len(rows), np.int32) if group is None else group[rows]
        with ieee_denormals():
            if desc:
                sub = fdr._grouped_q(s, t, g)
            else:
                sub = np.full(len(rows), np.nan)
                for gid in np.unique(g):
                    m = g == gid
                    sub[m] = fdr.tdc_qvalues(s[m], t[m], desc=False)
        q = np.full(n, np.nan)
        q[rows] = sub
        q.setflags(write=False)
        _host_q[name] = q
    return _host_q[name]


def host_labels(name: str, fdr: float) -> np.ndarray:
    """``_SemiSupervisedTDC._labels``' rule on ``host_q``: +1 used target with q <= fdr, 0 other target and
    every unused row, -1 used decoy."""
    _, target, _, use, _ = get(name)
    q = host_q(name)
    used = np.ones(len(q), bool) if use is None else use != 0
    lab = np.zeros(len(q), np.int8)
    lab[used & target & (q <= fdr)] = 1
    lab[used & ~target] = -1
    return lab


def get(name: str):
    """The case ``name`` of ``CASE_IDS``, built once; the arrays are shared and read-only."""
    if name not in _built:
        c = build(*dict(CASE_IDS)[name])
        for a in c[:4]:
            if a is not None:
                a.setflags(write=False)
        _built[name] = c
    return _built[name]
