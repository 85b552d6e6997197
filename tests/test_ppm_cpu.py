"""The yardstick of the ppm fragment tolerance and its cases, without a GPU.

* tests/ppm_ref.py, the per-peak-tolerance restatement of the shifted dot product, with a CONSTANT
  tolerance equals the CPU oracle bit for bit -- on the edge-planted blocks of tests/rescore_cases.py
  and on random spectra. That is what lets the GPU test hold the kernels against it in ppm mode,
  where the oracle has nothing to say.
* tests/ppm_cases.py plants what tests/test_gpu_ppm.py relies on: peaks inside, on and outside the
  ppm windows, gate candidates on both sides of the shift gate, and in every block pairs whose score
  no constant-width window reproduces.
* `Config.fragment_tolerance_unit`, its flag, and the flag word of the C ABI."""
import argparse

import numpy as np
import pytest

import ppm_cases as PC
import ppm_ref as PR
import rescore_cases as RC


# ------------------------------------------------------------------ the restatement is the oracle
def _same_as_oracle(O, queries, library, pairs, tol, shift):
    qo, qmz, qit, _, qpmz, _ = queries
    lo, lmz, lit, lch, lpmz, lz = library
    n_match = 0
    for q, r in pairs:
        a, b = slice(qo[q], qo[q + 1]), slice(lo[r], lo[r + 1])
        s0, m0 = O.dot_pair(qmz[a], qit[a], qpmz[q], lmz[b], lit[b], lch[b], lpmz[r], int(lz[r]), tol, shift)
        s1, m1 = PR.dot_pair(qmz[a], qit[a], qpmz[q], lmz[b], lit[b], lch[b], lpmz[r], int(lz[r]), tol, shift, 'Da')
        assert np.float64(s0).tobytes() == np.float64(s1).tobytes(), (q, r, s0, s1)
        assert np.array_equal(np.asarray(m0).reshape(-1, 2), m1), (q, r)
        n_match += len(m1)
    return n_match


@pytest.mark.parametrize('number', RC.REGIMES)
def test_constant_tolerance_equals_the_oracle_on_the_edge_blocks(O, number):
    """Every third planted pair of every block of the regime (all charges, shifts on): score bits and
    match list."""
    n = 0
    for block in RC.regime_blocks(number):
        pairs = [(int(block.owner[r]), r) for r in range(0, block.nlib, 3)]
        n += _same_as_oracle(O, block.queries, block.library, pairs, block.tol, True)
    assert n > 1000


@pytest.mark.parametrize('tol,shift', [(0.02, True), (0.4, True), (0.4, False), (0.0, True)])
def test_constant_tolerance_equals_the_oracle_on_random_spectra(O, tol, shift):
    """Spectra on a coarse grid (many generated matches, twice matched peaks at tol = 0.4), up to 250
    peaks, charges up to 6; and best_match's winner."""
    rng = np.random.default_rng(int(tol * 1000) + shift)

    def spectra(n, sizes, zmax):
        out = []
        for i in range(n):
            m = int(sizes[i % len(sizes)])
            g = np.sort(rng.choice(np.arange(200, 1800), size=m, replace=False)).astype(np.float32)
            mz = np.sort(g + rng.normal(0, 0.004, m).astype(np.float32))
            out.append((mz, rng.random(m).astype(np.float32), rng.integers(0, 4, m).astype(np.uint8)))
        return RC.pack(out, rng.uniform(400, 900, n), rng.integers(1, zmax + 1, n))
    library = spectra(40, [20, 50, 100, 129, 250], 6)
    queries = spectra(8, [1, 30, 100, 101, 250], 2)
    pairs = [(q, r) for q in range(8) for r in range(40)]
    assert _same_as_oracle(O, queries, library, pairs, tol, shift) > (1000 if tol else 0)
    L, Q = O.Spectra(*library), O.Spectra(*queries)
    rows = np.arange(40, dtype=np.int64)
    for q in range(8):
        b0, s0, m0 = O.best_match(Q, q, L, rows, tol, shift)
        b1, s1, m1 = PR.best_match(queries, q, library, rows, tol, shift, 'Da')
        assert (b0, s0) == (b1, s1) and np.array_equal(np.asarray(m0).reshape(-1, 2), m1)


def test_ranked_order():
    sc = [0.5, 0.9, 0.5, 0.9, 0.1]
    assert PR.ranked(sc, 3).tolist() == [1, 3, 0]
    assert PR.ranked(sc, 9).tolist() == [1, 3, 0, 2, 4]
    assert PR.ranked(sc, 2, keys=[9, 8, 7, 6, 5]).tolist() == [3, 1]      # ties by key (the library row)


# ------------------------------------------------------------------ the ppm blocks
def test_blocks_have_the_shapes_of_the_issue():
    blocks = PC.blocks()
    assert [b.ppm for b in blocks] == [5.0, 10.0, 20.0, 50.0, 0.2]
    for b in blocks:
        qo, qmz, _, _, qpmz, _ = b.queries
        lo, lmz, _, lch, lpmz, lz = b.library
        assert sorted(set(np.diff(qo).tolist())) == [1, 37, 100, 101]
        assert qmz.min() >= 100.0 and qmz.max() <= 2000.0
        cn = np.diff(lo)
        assert cn.min() >= 1 and (cn <= 64).sum() > 100 and ((cn >= 65) & (cn <= 80)).sum() >= 2 * b.nq
        assert cn.max() <= 80
        assert set(lz.tolist()) == {1, 2, 3, 4, 5, 8}
        assert 200 <= b.nlib <= 400 and b.nq == 16
        for o, mz in ((qo, qmz), (lo, lmz)):
            inner = np.ones(len(mz), bool)
            inner[o[1:-1]] = False
            assert np.all(np.diff(mz)[inner[1:]] >= 0) and np.all(mz > 0), 'peaks ascend'
        assert np.all(lch <= lz[np.repeat(np.arange(b.nlib), cn)])
        # one gate candidate per query, on either side of the threshold in every block, within an ulp
        g = np.nonzero(b.gate)[0]
        assert len(g) == b.nq and sorted(b.owner[g].tolist()) == list(range(b.nq))
        assert (b.gate[g] > 0).any() and (b.gate[g] < 0).any()
        for r in g:
            q = int(b.owner[r])
            thr = PR.shift_gate(qpmz[q], b.ppm, 'ppm')
            S, pmd = PR.num_shifts(qpmz[q], lpmz[r], int(lz[r]), b.ppm, True, 'ppm')
            assert abs(abs(pmd) - thr) <= np.spacing(thr)
            assert S == (int(lz[r]) + 1 if b.gate[r] > 0 else 1)
            assert (abs(pmd) >= thr) == (b.gate[r] > 0)
    # the deferred block: its widest window lies below what the bin filter hashes at m/z 2000
    d = blocks[-1]
    assert float(PR.rel_tol(d.ppm)) * float(d.queries[1].max()) < RC.threshold_tol(2000.0)
    for b in blocks[:-1]:
        for q in range(b.nq):
            top = float(b.queries[1][b.queries[0][q + 1] - 1])
            assert RC.margin(float(PR.rel_tol(b.ppm)) * top, top) <= RC.RS_MARGIN_MAX


@pytest.mark.parametrize('i', range(5))
def test_block_plants_peaks_inside_on_and_outside(i):
    b = PC.blocks()[i]
    inside, outside, on = PC.window_stats(b)
    print(f'{b.name}: {b.nlib} pairs; within 4 ulp of an edge: {inside} inside, {outside} outside; {on} on it')
    # what the generator must reach at the least: a block plants about 11 000 peaks (240 candidates of
    # 32 .. 80), one in 17 of them at k = 20, i.e. tol_i * 2^-20 <= 1e-7 from the exact edge -- far less
    # than a float32 ulp at m/z >= 100 (7.6e-6) -- so about 650 peaks are the float32 nearest to an edge
    # before the nudge of -2 .. +2 ulps moves two fifths of them inside, two fifths outside, and leaves a fifth
    assert inside >= 250 and outside >= 250 and on >= 100


@pytest.mark.parametrize('i', range(5))
def test_no_constant_width_reproduces_a_block(i):
    """Scores at tol_i against Da runs at the window of the lowest and of the highest query m/z of the
    block: each differs on at least ten pairs, so a constant-width implementation cannot pass the GPU
    test; and the block holds matched peaks by the thousand and pairs with a doubly matched peak."""
    b = PC.blocks()[i]
    qmz = b.queries[1]
    lo_da = float(PR.rel_tol(b.ppm) * np.float64(qmz.min()))
    hi_da = float(PR.rel_tol(b.ppm) * np.float64(qmz.max()))
    n_lo = n_hi = n_match = twice = 0
    for r in range(b.nlib):
        q = int(b.owner[r])
        s, m = PR.pair(b.queries, q, b.library, r, b.ppm, True, 'ppm')
        n_lo += s != PR.pair(b.queries, q, b.library, r, lo_da, True, 'Da')[0]
        n_hi += s != PR.pair(b.queries, q, b.library, r, hi_da, True, 'Da')[0]
        n_match += len(m)
        qs = PR.spectrum(b.queries, q)
        cs = PR.spectrum(b.library, r)
        gi, _, ci, _ = PR.generated(qs[0], qs[3], cs[0], cs[2], cs[3], cs[4], b.ppm, True, 'ppm')
        twice += len(gi) > len(m)
    print(f'{b.name}: {n_match} matched peaks; {n_lo} / {n_hi} of {b.nlib} pairs differ from Da at the '
          f'lowest / highest window; {twice} pairs with a doubly matched peak')
    assert n_lo >= 10 and n_hi >= 10
    assert n_match >= 1000 and twice >= 10


# ------------------------------------------------------------------ configuration
def test_config_validation_and_flag():
    from ann_solo_amd.config import Config, add_arguments
    assert Config().fragment_tolerance_unit == 'Da'
    assert Config(fragment_tolerance_unit='ppm', fragment_mz_tolerance=10).fragment_tolerance_unit == 'ppm'
    for bad in ('PPM', 'da', '', None, 1):
        with pytest.raises(ValueError, match='fragment_tolerance_unit'):
            Config(fragment_tolerance_unit=bad)
    with pytest.raises(ValueError, match='num_gpus'):
        Config(fragment_tolerance_unit='ppm', num_gpus=2)
    assert Config(fragment_tolerance_unit='Da', num_gpus=2).num_gpus == 2
    assert Config(fragment_tolerance_unit='ppm', num_gpus=1).fragment_tolerance_unit == 'ppm'
    p = argparse.ArgumentParser()
    add_arguments(p)
    assert p.parse_args([]).fragment_tolerance_unit == 'Da'
    ns = p.parse_args(['--fragment_tolerance_unit', 'ppm'])
    assert Config.from_reference(ns).fragment_tolerance_unit == 'ppm'
    with pytest.raises(SystemExit):
        p.parse_args(['--fragment_tolerance_unit', 'mmu'])
    # the reference's own flag is NOT this option: its 'ppm' default must not switch the mode on
    ref = argparse.Namespace(fragment_tol_mode='ppm', fragment_mz_tolerance=0.02)
    assert Config.from_reference(ref).fragment_tolerance_unit == 'Da'


def test_flag_word():
    import os
    import re
    from ann_solo_amd import spectrum_match as sm
    assert [sm.score_flags(a, u) for a in (False, True) for u in ('Da', 'ppm')] == [0, 2, 1, 3]
    assert sm.score_flags(7, 'Da') == 1 and sm.score_flags(np.bool_(True)) == 1
    with pytest.raises(ValueError):
        sm.score_flags(True, 'PPM')
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                           'annsolo_mi.h')) as f:
        header = f.read()
    assert int(re.search(r'#define ASL_SCORE_SHIFT (\d+)', header).group(1)) == sm.SCORE_SHIFT == 1
    assert int(re.search(r'#define ASL_SCORE_FRAGMENT_PPM (\d+)', header).group(1)) == sm.SCORE_FRAGMENT_PPM == 2
